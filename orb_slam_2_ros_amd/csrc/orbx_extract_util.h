// orbx_extract_util.h -- what more than one stage of the ORB extractor
// (orbx_pyramid.hip, orbx_fast.hip, orbx_quadtree.hip, orbx_describe.hip)
// uses: level addressing, the XCD block mapping, lane / scan helpers, the
// wave-cooperative LDS staging and the phase-profiling marks.
// Every launch covers a whole batch of frames (grid.y / grid.z = frame).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <type_traits>

#include "orbx_device.h"
#include "orbx_math.h"
#include "orbx_wave.h"

namespace orbx {

// Phase profiling (diagnostic build only, -DORBX_PHASE_PROF: tools/phase_prof.py):
// each wave adds the s_memtime cycles of its phases to g_phase[phase] (lane 0,
// vector atomics).  The product build compiles the marks away.
// Each profiled stage's file (k_fast, k_describe, k_quadtree) defines its own
// g_phase[8][256] and a host reader (a __device__ array cannot span
// translation units without relocatable device code); PHASE_MARK's K names the
// kernel's place in orbx_debug_phase_cycles' output (0 fast, 1 describe,
// 2 quadtree) and is otherwise unused.
#ifdef ORBX_PHASE_PROF
// (256 slots per counter, by workgroup: one shared address per counter would
// serialise every wave's atomic at one L2 channel)
#define PHASE_START() uint64_t phase_t_ = __builtin_amdgcn_s_memtime()
#define PHASE_MARK(K, I)                                                                  \
    do {                                                                                  \
        const uint64_t phase_n_ = __builtin_amdgcn_s_memtime();                          \
        if ((threadIdx.x & 63) == 0)                                                      \
            atomicAdd(&g_phase[I][(blockIdx.x + 37 * blockIdx.y) & 255],                 \
                      (unsigned long long)(phase_n_ - phase_t_));                         \
        phase_t_ = phase_n_;                                                              \
    } while (0)
// out[0..8) = a stage's eight counters, each summed over its 256 slots; reset zeroes them.
inline hipError_t phase_read(const void *sym, unsigned long long *out, bool reset) {
    static unsigned long long h[8 * 256];
    if (hipMemcpyFromSymbol(h, sym, sizeof(h)) != hipSuccess) return hipErrorInvalidValue;
    for (int i = 0; i < 8; ++i) {
        out[i] = 0;
        for (int j = 0; j < 256; ++j) out[i] += h[256 * i + j];
    }
    if (!reset) return hipSuccess;
    static const unsigned long long z[8 * 256] = {};
    return hipMemcpyToSymbol(sym, z, sizeof(z));
}
hipError_t phase_cycles_fast(unsigned long long *out, bool reset);
hipError_t phase_cycles_describe(unsigned long long *out, bool reset);
hipError_t phase_cycles_quadtree(unsigned long long *out, bool reset);
#else
#define PHASE_START() uint64_t phase_t_ = 0; (void)phase_t_
#define PHASE_MARK(K, I) (void)0
#endif

// Per-phase instruction counts (tools/phase_valu.sh): a build with
// -DORBX_STOP_FAST=N / -DORBX_STOP_DESC=N compiles k_fast / k_describe only up
// to the end of phase N (k_fast: 1 staging, 2 iniThFAST compass + compaction,
// 3 its arc scores, 4 its NMS + output, no minThFAST pass; k_describe:
// 1 staging, 2 moments + row pass, 4 orientation + sample offsets + column
// pass), so SQ_INSTS_* differences between builds split the counts by phase.
// Results of such builds are wrong by design; 0 = the product.
#ifndef ORBX_STOP_FAST
#define ORBX_STOP_FAST 0
#endif
#ifndef ORBX_STOP_DESC
#define ORBX_STOP_DESC 0
#endif
constexpr int kStopFast = ORBX_STOP_FAST, kStopDesc = ORBX_STOP_DESC;

namespace {

constexpr int kThreads = 256;

__device__ inline const uint8_t *level_ptr(const DevPlan &p, const FrameBufs &fb, const LevelGeom &g,
                                           int l, int b, int &pitch) {
    if (l == 0) {
        pitch = fb.img0_pitch;
        return fb.img0 + (int64_t)b * fb.img0_stride;
    }
    pitch = g.pitch;
    return fb.pyr + (int64_t)b * p.pyr_bytes + g.pyr_off;
}

__device__ inline const uint8_t *level_ptr(const DevPlan &p, const FrameBufs &fb, int l, int b, int &pitch) {
    if (l == 0) {
        pitch = fb.img0_pitch;
        return fb.img0 + (int64_t)b * fb.img0_stride;
    }
    pitch = p.la[l].pitch;
    return fb.pyr + (int64_t)b * p.pyr_bytes + p.la[l].pyr_off;
}

// The dispatcher hands workgroup j (linear, x fastest) to XCD j % 8.  This
// maps j to a logical block index so that each XCD runs a contiguous range of
// logical blocks: consecutive blocks of one frame then share an XCD's L2
// (overlapping cell rings / keypoint patches hit instead of refetching).
constexpr int kXcds = 8;
__device__ inline int xcd_logical_block(int j, int n) {
    const int per = (int)((uint32_t)n / kXcds), rem = (int)((uint32_t)n % kXcds), xcd = (int)((uint32_t)j % kXcds),
              idx = (int)((uint32_t)j / kXcds);
    return xcd < rem ? xcd * (per + 1) + idx : rem * (per + 1) + (xcd - rem) * per + idx;
}

// (x, y) of the logical block of a 2-D grid, the division by gridDim.x as a
// multiply-high by a host-made magic ceil(2^32 / gridDim.x) (grid_magic), exact
// while (blocks) x gridDim.x < 2^32 (checked by the launcher; magic 0 = divide):
// 3 scalar instructions instead of the ~20 of a 32-bit division.
__device__ inline void xcd_block_2d(int &bx, int &by, uint32_t magic) {
    const int n = gridDim.x * gridDim.y;
    const int L = xcd_logical_block(blockIdx.y * gridDim.x + blockIdx.x, n);
    by = magic ? (int)__umulhi((uint32_t)L, magic) : L / (int)gridDim.x;
    bx = L - by * (int)gridDim.x;
}

// The wave's index in its workgroup as a scalar: the compiler cannot prove
// threadIdx.x >> 6 wave-uniform, so everything derived from it would live in
// VGPRs and branch per lane.
__device__ inline int wave_id() { return __builtin_amdgcn_readfirstlane(threadIdx.x >> 6); }
// set bits of m below this lane (v_mbcnt_lo / hi: two VALU, where a masked popcount takes four)
// The lane mask of a comparison straight from its v_cmp (an SGPR pair).
// __ballot of a bool that also steers a branch is lowered as v_cndmask 0 / 1
// plus a second v_cmp; these keep the compare's own mask.
__device__ inline uint64_t lanes_lt(int a, int b) { return __builtin_amdgcn_sicmp(a, b, 40); }   // ICMP_SLT
__device__ inline uint64_t lanes_gt(int a, int b) { return __builtin_amdgcn_sicmp(a, b, 38); }   // ICMP_SGT

__device__ inline int mbcnt64(uint64_t m) {
    return (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}

__device__ inline uint32_t pack_key(int x, int y, int score) {
    return (uint32_t)x | ((uint32_t)y << 12) | ((uint32_t)score << 24);
}

// ---- wave / block helpers (wave64) ----------------------------------------
// Exclusive scan of a[0..m) (uint64) in LDS by the whole NT-thread block.
// ws: NT / 64 uint64 of LDS scratch.  Returns the total.  Ends with a barrier.
template <int NT = kThreads>
__device__ uint64_t block_excl_scan_u64(uint64_t *a, int m, uint64_t *ws) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int per = (m + NT - 1) / NT;
    const int s = min(tid * per, m), e = min(s + per, m);
    uint64_t local = 0;
    for (int i = s; i < e; ++i) local += a[i];
    const uint64_t incl = wave_incl_scan_u64(local);
    if (lane == 63) ws[wave] = incl;
    __syncthreads();
    uint64_t base = 0, total = 0;
    for (int w = 0; w < NT / 64; ++w) {
        if (w < wave) base += ws[w];
        total += ws[w];
    }
    uint64_t run = base + incl - local;
    for (int i = s; i < e; ++i) {
        const uint64_t v = a[i];
        a[i] = run;
        run += v;
    }
    __syncthreads();
    return total;
}

// Unsigned 24-bit multiply (v_mul_u32_u24, full rate); both operands must be
// in [0, 2^24), which every use below guarantees.
// (__umul24: the masked-product form let the compiler pick v_mul_lo_u32, a
// quarter-rate op, whenever one operand was a scalar it had proven small)
__device__ inline int mul24u(int a, int b) { return (int)__umul24((uint32_t)a, (uint32_t)b); }

// Small exact integer division for the index walks (a < 2^15, b <= 255).
__device__ inline int div_small(int a, int b) {
    return (int)(((float)a + 0.5f) * __builtin_amdgcn_rcpf((float)b));
}

// ===========================================================================
// Wave-cooperative staging of an image rectangle into LDS with aligned dword
// loads, NB in flight per lane before any LDS store (a rectangle of up to
// 64 * NB dwords costs one global round trip).  Pixel (r, c) of the
// rectangle lands at dst[r * ds + o + c]; returns o = x0 & 3.  The caller
// guarantees a 4-aligned image base and pitch and that the aligned span
// [x0 & ~3, x0 + nc rounded up to 4) lies inside the row's pitch.
// ===========================================================================
template <int NB = 8>
__device__ inline int wave_stage_rect(uint8_t *dst, int ds, const uint8_t *img, int pitch, int y0, int x0,
                                      int nr, int nc, int lane) {
    const int xa = x0 & ~3, o = x0 - xa;
    const int nd = (o + nc + 3) >> 2;
    const int total = nr * nd;
    const int dr = div_small(64, nd), dk = 64 - dr * nd;
    const int r_l = div_small(lane, nd), k_l = lane - r_l * nd;
    const uint8_t *base = img + (int64_t)y0 * pitch + xa;
    for (int i0 = 0, r0 = r_l, k0 = k_l; i0 < total; i0 += 64 * NB) {
        uint32_t v[NB];
        int r = r0, k = k0;
#pragma unroll
        for (int j = 0; j < NB; ++j) {
            if (i0 + 64 * j + lane < total) v[j] = *reinterpret_cast<const uint32_t *>(base + mul24u(r, pitch) + 4 * k);
            r += dr; k += dk; if (k >= nd) { k -= nd; ++r; }
        }
        r = r0; k = k0;
#pragma unroll
        for (int j = 0; j < NB; ++j) {
            if (i0 + 64 * j + lane < total) *reinterpret_cast<uint32_t *>(dst + mul24u(r, ds) + 4 * k) = v[j];
            r += dr; k += dk; if (k >= nd) { k -= nd; ++r; }
        }
        r0 = r; k0 = k;
    }
    return o;
}


// A raw buffer resource over a wave-uniform base: loads through it take a
// 32-bit per-lane offset plus a scalar offset, so no 64-bit address
// arithmetic runs on the VALU (2 VALU per global_load otherwise).  The range
// check is left open (the callers never read past their rectangles).
__device__ inline __amdgpu_buffer_rsrc_t wave_rsrc(const void *base) {
    const uint64_t a = reinterpret_cast<uint64_t>(base);
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)a);
    const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)(a >> 32));
    return __builtin_amdgcn_make_buffer_rsrc(reinterpret_cast<void *>(((uint64_t)hi << 32) | lo), (short)0,
                                             0x7FFFFFF0, 0x00020000);
}

__device__ inline uint32_t buf_ld32(__amdgpu_buffer_rsrc_t r, int voff, int soff) {
    return __builtin_amdgcn_raw_buffer_load_b32(r, voff, soff, 0);
}

// The same staging with a fixed lane -> (row in pass, dword) map, so each
// load's address is one uniform row offset plus a fixed per-lane offset (no
// per-load index walk): rows of at most 64 dwords go 64 / nd rows per pass;
// wider rows one row per pass in 64-dword chunks, NB rows per round.  BUF:
// buffer loads, the row offset a scalar operand and the lane offset a 32-bit
// VGPR (k_fast, k_describe: -2 % time); the resize windows (up to 24
// rows in flight) measured 2 % slower that way and keep global loads.
// X80: the bytes are stored XOR 0x80 (as signed I - 128, k_describe's int8 MFMAs).
// FO >= 0 (BUF only): the rectangle lands at dst column FO whatever x0's
// alignment (the loads are then unaligned dwords from x0 - FO; the buffer
// base stays 4-aligned and the remainder goes into the lane offset).
template <int NB = 8, bool BUF = true, bool X80 = false, int FO = -1>
__device__ inline int wave_stage_rows(uint8_t *dst, int ds, const uint8_t *img, int pitch, int y0, int x0, int nr,
                                      int nc, int lane) {
    constexpr uint32_t kX = X80 ? 0x80808080u : 0u;
    static_assert(FO < 0 || BUF, "a forced column offset needs the buffer loads");
    // (all wave-uniform: row offsets then come from the scalar unit)
    pitch = __builtin_amdgcn_readfirstlane(pitch);
    ds = __builtin_amdgcn_readfirstlane(ds);
    nr = __builtin_amdgcn_readfirstlane(nr);
    const int xs = FO >= 0 ? x0 - FO : x0;                  // first byte loaded
    const int xa = xs & ~3, o = FO >= 0 ? FO : x0 - xa;
    const int sh = FO >= 0 ? xs - xa : 0;                   // load misalignment
    const int nd = (o + nc + 3) >> 2;
    const uint8_t *gsrc = img + (int64_t)y0 * pitch + xa;
    const __amdgpu_buffer_rsrc_t src = wave_rsrc(gsrc);
    auto load = [&](int voff, int row) -> uint32_t {
        if constexpr (BUF) return buf_ld32(src, voff, __builtin_amdgcn_readfirstlane(row * pitch));
        else return *reinterpret_cast<const uint32_t *>(gsrc + mul24u(row, pitch) + voff);
    };
    if (nd > 64) {
        for (int c0 = 0; c0 < nd; c0 += 64) {
            const bool on = c0 + lane < nd;
            const int voff = 4 * (c0 + lane) + sh;
            for (int r0 = 0; r0 < nr; r0 += NB) {
                uint32_t v[NB];
#pragma unroll
                for (int j = 0; j < NB; ++j)
                    if (on && r0 + j < nr) v[j] = load(voff, r0 + j);
#pragma unroll
                for (int j = 0; j < NB; ++j)
                    if (on && r0 + j < nr) *reinterpret_cast<uint32_t *>(dst + mul24u(r0 + j, ds) + voff - sh) = v[j] ^ kX;
            }
        }
        return o;
    }
    const int R = __builtin_amdgcn_readfirstlane(div_small(64, nd));   // rows per pass (wave-uniform)
    const int rl = div_small(lane, nd), k = lane - mul24u(rl, nd);
    const int voff = mul24u(rl, pitch) + 4 * k + sh, loff = mul24u(rl, ds) + 4 * k;
    const int rmax = rl < R ? nr - rl : 0;   // this lane loads rows r0 + j R < rmax
    // the row offsets as scalar multiples of R * pitch (a v_mul_lo_u32 per
    // load otherwise: quarter rate, then a readfirstlane)
    const int Rp = __builtin_amdgcn_readfirstlane(R * pitch);
    for (int r0 = 0, s0 = 0; r0 < nr; r0 += NB * R, s0 += NB * Rp) {
        uint32_t v[NB];
#pragma unroll
        for (int j = 0; j < NB; ++j) {
            if constexpr (BUF) {
                if (r0 + mul24u(j, R) < rmax) v[j] = buf_ld32(src, voff, s0 + j * Rp);
            } else {
                if (r0 + j * R < rmax) v[j] = load(voff, r0 + j * R);
            }
        }
#pragma unroll
        for (int j = 0; j < NB; ++j)
            if constexpr (BUF) {
                if (r0 + mul24u(j, R) < rmax) *reinterpret_cast<uint32_t *>(dst + mul24u(r0 + mul24u(j, R), ds) + loff) = v[j] ^ kX;
            } else {
                if (r0 + j * R < rmax) *reinterpret_cast<uint32_t *>(dst + mul24u(r0 + j * R, ds) + loff) = v[j] ^ kX;
            }
    }
    return o;
}

typedef __attribute__((address_space(3))) uint8_t lds_u8;   // LDS byte (keeps ds_read_u8)
typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
__device__ inline u16x2 as_u16x2(uint32_t v) { return __builtin_bit_cast(u16x2, v); }

// Magic for xcd_block_2d(bx, by, magic): ceil(2^32 / gx), exact for every
// block index L with L * gx < 2^32; 0 (divide) when that does not hold.
uint32_t grid_magic(uint32_t gx, uint32_t gy) {
    if (gx <= 1 || (uint64_t)gx * gy * gx >= (1ull << 32)) return 0;
    return (uint32_t)(((1ull << 32) + gx - 1) / gx);
}

// Dynamic LDS above 64 KiB must be opted into per kernel.
template <typename K>
hipError_t allow_lds(K kernel, int bytes) {
    if (bytes <= 64 * 1024) return hipSuccess;
    return hipFuncSetAttribute(reinterpret_cast<const void *>(kernel),
                               hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
}

}  // namespace

}  // namespace orbx
