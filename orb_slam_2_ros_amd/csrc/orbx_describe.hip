// orbx_describe.hip -- orientation and rBRIEF of the ORB extractor on gfx950.
//
// Stage                       reference (wjjcdy/orb_slam_2_ros)
//   k_blur     (all levels)   GaussianBlur 7x7 s=2, ORBextractor.cc:1128-1130
//   k_describe (one wave/kp)  IC_Angle + computeOrbDescriptor + scaling,
//                             ORBextractor.cc:77-147, 1116-1148
// k_describe runs its orientation moments and blur row pass as int8 MFMAs
// (15 per keypoint); k_blur writes the blurred levels only for the debug /
// reference path (k_describe blurs patch-locally).
#include "orbx_extract_util.h"

namespace orbx {

// rBRIEF sampling points (ORBextractor.cc:150-408)
constexpr int kPatternPts[512][2] = {
#define ORBX_PATTERN_BEGIN
#define ORBX_PATTERN_END
#include "orb_pattern.inc"
#undef ORBX_PATTERN_BEGIN
#undef ORBX_PATTERN_END
};
// The descriptor's rotation multiplies them in float; k_describe fetches them
// as OCP fp8 e4m3fn (gfx950's format: every integer of magnitude <= 16 is
// exact) and widens a point (x, y) to an f32 pair with one
// v_cvt_pk_f32_fp8: lane l's 16 bytes are pairs 64 g + l, g = 0..3, as
// (x0, y0, x1, y1) -- one 16-byte load a lane instead of four.
constexpr uint32_t fp8_e4m3_int(int n) {   // n in [-15, 15]
    int a = n < 0 ? -n : n, e = 0;
    while (a >> (e + 1)) ++e;
    return n == 0 ? 0u : (uint32_t)((n < 0 ? 0x80 : 0) | ((e + 7) << 3) | (((a << 3) >> e) & 7));
}
struct PatternQ {
    uint32_t w[64][4];
    constexpr PatternQ() : w() {
        for (int l = 0; l < 64; ++l)
            for (int g = 0; g < 4; ++g) {
                const int j = 64 * g + l;
                w[l][g] = fp8_e4m3_int(kPatternPts[2 * j][0]) | fp8_e4m3_int(kPatternPts[2 * j][1]) << 8 |
                          fp8_e4m3_int(kPatternPts[2 * j + 1][0]) << 16 | fp8_e4m3_int(kPatternPts[2 * j + 1][1]) << 24;
            }
    }
};
constexpr bool pattern_in_fp8_range() {
    for (int i = 0; i < 512; ++i)
        for (int c = 0; c < 2; ++c)
            if (kPatternPts[i][c] < -15 || kPatternPts[i][c] > 15) return false;
    return true;
}
static_assert(pattern_in_fp8_range(), "the fp8 pattern table holds integers up to 15 exactly");
static_assert(fp8_e4m3_int(1) == 0x38 && fp8_e4m3_int(13) == 0x55 && fp8_e4m3_int(-3) == 0xC4, "e4m3fn, bias 7");

// c_disc_mask[ri][g]: byte k kept iff column 4g - 16 + k lies in row ri - 15
// of the orientation disc (kUmax, orbx_plan.h).
struct DiscMask {
    uint32_t m[32][8];
    constexpr DiscMask() : m() {
        for (int ri = 0; ri < 32; ++ri)
            for (int g = 0; g < 8; ++g) {
                uint32_t keep = 0;
                const int v = ri - 15, av = v < 0 ? -v : v;
                for (int k = 0; k < 4; ++k) {
                    const int u = 4 * g - 16 + k, au = u < 0 ? -u : u;
                    if (ri < 31 && au <= kUmax[av]) keep |= 0xFFu << (8 * k);
                }
                m[ri][g] = keep;
            }
    }
};
__constant__ DiscMask c_disc_mask = DiscMask();

// IC_Angle's moments on the matrix cores (k_describe): three int8 MFMAs over
// the staged patch (rows 0..47 as three 16-row tiles; the keypoint at patch
// column 23, so the disc, rows 6..36 and columns 8..38, lies in one 32-column
// window, columns 8..39).  Per (row tile rt, lane):
//   mask: the A-operand bytes kept, patch row 16 rt + (l & 15), window
//         columns 8 (l >> 4) + 0..7, inside the disc (kUmax);
//   b:    the B-operand bytes, k = 8 (l >> 4) + 0..7, output column j = l & 15:
//         j = 15: u = k - 15 (m10), j = 12 + rt: 1 (the rows' sums, weighted
//         by their v afterwards: m01), others 0.
constexpr int kDescKpCol = 23;   // the keypoint's patch column (k_describe staging)
struct MomTables {
    uint64_t mb[3][64][2];   // (mask, b): one 16-byte load a product
    constexpr MomTables() : mb() {
        for (int rt = 0; rt < 3; ++rt)
            for (int l = 0; l < 64; ++l) {
                uint64_t mk = 0, bb = 0;
                const int v = 16 * rt + (l & 15) - 21, av = v < 0 ? -v : v, j = l & 15;
                for (int jj = 0; jj < 8; ++jj) {
                    const int u = 8 + 8 * (l >> 4) + jj - kDescKpCol, au = u < 0 ? -u : u;
                    if (av <= 15 && au <= kUmax[av]) mk |= 0xFFull << (8 * jj);
                    const int w = j == 15 ? u : (j == 12 + rt ? 1 : 0);
                    bb |= (uint64_t)(uint8_t)(int8_t)w << (8 * jj);
                }
                mb[rt][l][0] = mk;
                mb[rt][l][1] = bb;
            }
    }
};

#ifdef ORBX_PHASE_PROF
// this stage's phase counters (orbx_extract_util.h); slots 8..15 of orbx_debug_phase_cycles
namespace {
__device__ unsigned long long g_phase[8][256];
}  // namespace
hipError_t phase_cycles_describe(unsigned long long *out, bool reset) { return phase_read(&g_phase, out, reset); }
#endif

namespace {

__device__ inline int reflect101(int v, int n) {
    // BORDER_REFLECT_101 for the 3-px halo of a >= 4 px image.
    v = v < 0 ? -v : v;
    return v >= n ? 2 * n - v - 2 : v;
}

// ===========================================================================
// K2: Gaussian 7x7, sigma 2, BORDER_REFLECT_101 on each level (OpenCV 3.2
// fixed-point separable filter).  The SSE2 column pass accumulates exactly in
// float and rounds half-to-even; the scalar tail adds 2^15 and shifts: both are
// reproduced here in integers (exact: the float sums are < 2^24 whenever the
// result is < 256).  Tile = 64 x 16 outputs, 70 x 22 inputs in LDS.
// ===========================================================================
constexpr int kBlurTW = 64, kBlurTH = 16;

__global__ __launch_bounds__(kThreads) void k_blur(DevPlan p, FrameBufs fb) {
    const int4 t = p.blur_tiles[blockIdx.x];
    const int l = t.x, x0 = t.y, y0 = t.z, b = blockIdx.y;
    const LevelGeom g = p.lv[l];
    int spitch;
    const uint8_t *src = level_ptr(p, fb, g, l, b, spitch);
    uint8_t *dst = fb.blur + (int64_t)b * p.blur_bytes + g.blur_off;
    __shared__ uint8_t tin[kBlurTH + 6][kBlurTW + 8];
    __shared__ int rowp[kBlurTH + 6][kBlurTW];
    const int tid = threadIdx.x;
    for (int i = tid; i < (kBlurTH + 6) * (kBlurTW + 6); i += kThreads) {
        const int r = i / (kBlurTW + 6), c = i - r * (kBlurTW + 6);
        const int yy = reflect101(min(y0 + r - 3, g.h + 2), g.h);
        const int xx = reflect101(min(x0 + c - 3, g.w + 2), g.w);
        tin[r][c] = src[(int64_t)yy * spitch + xx];
    }
    __syncthreads();
    const int k0 = p.gauss[0], k1 = p.gauss[1], k2 = p.gauss[2], k3 = p.gauss[3];
    for (int i = tid; i < (kBlurTH + 6) * kBlurTW; i += kThreads) {
        const int r = i / kBlurTW, c = i - r * kBlurTW;
        const uint8_t *q = &tin[r][c];
        rowp[r][c] = k0 * (q[0] + q[6]) + k1 * (q[1] + q[5]) + k2 * (q[2] + q[4]) + k3 * q[3];
    }
    __syncthreads();
    const int xs = g.w & ~3;
    for (int i = tid; i < kBlurTH * kBlurTW; i += kThreads) {
        const int r = i / kBlurTW, c = i - r * kBlurTW;
        const int x = x0 + c, y = y0 + r;
        if (x >= g.w || y >= g.h) continue;
        const int s = k3 * rowp[r + 3][c] + k2 * (rowp[r + 2][c] + rowp[r + 4][c]) +
                      k1 * (rowp[r + 1][c] + rowp[r + 5][c]) + k0 * (rowp[r][c] + rowp[r + 6][c]);
        int q = s >> 16;
        if (x < xs) {
            const int rem = s & 0xFFFF;
            q += (rem > 0x8000) | ((rem == 0x8000) & (q & 1));
        } else {
            q = (s + (1 << 15)) >> 16;
        }
        dst[(int64_t)y * g.pitch + x] = (uint8_t)min(q, 255);
    }
}

// ===========================================================================
// K5: orientation + rBRIEF + keypoint record, one wave per selected key.
// The wave stages the 43x43 neighbourhood of its keypoint (radius 21, with the
// level's reflect-101 at the borders) in LDS once; from it come the integer
// IC moments (radius-15 disc, unblurred), the horizontal pass of the 7x7 s=2
// Gaussian over the window the rotated pattern can reach (|offset| <= 18), and
// each of the 512 samples as the vertical pass at that pixel.  Identical to
// sampling the blurred level (same taps, same per-column rounding); no
// blurred pyramid is written to HBM.
// ===========================================================================
constexpr int kDescR = 21;                  // patch radius = 18 (samples) + 3 (blur taps)
constexpr int kDescP = 2 * kDescR + 1;      // 43
constexpr int kDescPS = 48;                 // patch row stride (bytes): 43 + align offset, 8-aligned rows
constexpr int kBlurR = 18;
constexpr int kRowCols = 40;                // row-pass outputs at patch columns 0..39
constexpr int kColS = 44;                   // column-major row-pass buffer: stride (u16) of a column, rows 0..43
// The row-pass buffer is column-major: a sample's seven column-pass inputs
// (rows r..r+6 of one column) are 14 contiguous bytes, one unaligned
// ds_read_b128 (row 43 is padding the read may cover).
// The MFMA row pass reads 48 rows x 64 columns at the patch stride (rows
// 43..47, and columns past 45 that wrap into the next row, are either
// multiplied by zero taps or feed outputs that are never stored), all of it
// into registers before its first store: the patch is dead by then, so the
// row buffer overlays it (kDescRowOff = 0; 3.5 KB a wave instead of 5.5:
// LDS no longer caps the occupancy).
constexpr int kDescWaves = 8;    // waves per SIMD the launch bounds ask for (VGPR budget 512 / this)
// Waves (consecutive keypoint slots of a frame) per workgroup.  The waves share
// nothing, so the width only sets how many wave slots and how much LDS are
// taken and given back at once: one-wave workgroups measured fastest
// (k_describe per 3072 VGA frames: 2.40 ms with four waves and their
// orientations on wave 0, 2.30 with four and 2.20 with one wave each
// evaluating its own; profiles/r07_ab_describe.txt)
constexpr int kDescW = 1;
constexpr int kDescThreads = 64 * kDescW;
constexpr int kDescRowOff = 0;   // the row buffer's offset in the wave's LDS: over the patch
constexpr int kDescWaveLds = std::max(kDescRowOff + kRowCols * kColS * 2 + 8,    // (+ 8: the row pass's spill, below)
                                      47 * kDescPS + 64);                         // 3528 B
static_assert((kDescR - 3 + kBlurR) + 7 < kColS, "a sample's 16-byte read stays in its column");
constexpr int kDescWaveStride = (kDescWaveLds + 15) & ~15;
static_assert(47 * kDescPS + 63 < kDescWaveLds, "MFMA row-pass reads stay inside the wave's LDS");
// A CU holds 4 kDescWaves = 32 waves, that is 32 / kDescW workgroups.  LDS is
// allocated per workgroup in 512-byte granules (3584 B for the one wave's 3536):
// that many workgroups must fit a CU's 160 KB (32 x 3584 B = 112 KB)
static_assert((4 * kDescWaves) % kDescW == 0 && kDescThreads <= 1024, "whole workgroups fill the CU's wave slots");
static_assert(4 * kDescWaves / kDescW * ((kDescW * kDescWaveStride + 511) & ~511) <= 160 * 1024,
              "k_describe: LDS for the occupancy the launch bounds ask");
static_assert(kDescW * kDescWaveStride <= 64 * 1024, "static LDS of one workgroup");

// The row pass as an int8 matrix product (v_mfma_i32_16x16x32_i8): outputs
// j = 0..15 of a 16-column tile from the tile's 32 input columns,
//   R[r][16 t + j] = sum_c T[j][c] P[r][16 t + c],  T[j][c] = w[c - j] (0 <= c - j <= 6).
// T is the A operand, lane l holds T[l & 15][8 (l >> 4) + 0..7] (8 bytes, i8:
// the taps are <= 55).  The pixels go in as P - 128 (xor 0x80), so the
// accumulator starts at 128 * sum(w) = 128 * 257 = 32896, and the exact i32
// result is the reference's integer row sum (<= 65535).
struct RowTaps {
    uint64_t t[64];
    constexpr RowTaps() : t() {
        for (int l = 0; l < 64; ++l) {
            uint64_t v = 0;
            for (int jj = 0; jj < 8; ++jj) {
                const int d = 8 * (l >> 4) + jj - (l & 15);
                if (d >= 0 && d <= 6) v |= (uint64_t)kGaussTaps[d] << (8 * jj);
            }
            t[l] = v;
        }
    }
};
// k_describe's three per-lane tables in one constant block: one buffer
// resource (one s_getpc / add / addc) serves every table load at immediate offsets
struct DescTables {
    MomTables mom;   // 3072 B
    PatternQ pat;    // 1024 B
    RowTaps taps;    // 512 B
};
static_assert(offsetof(DescTables, pat) == 3072 && offsetof(DescTables, taps) == 4096, "immediate offsets below");
__constant__ __attribute__((aligned(16))) DescTables c_desc = DescTables();
typedef int i32x4 __attribute__((ext_vector_type(4)));

// k_describe's 43 x 43 patch inside the level, staged with its column 0 at
// patch column 2 (the keypoint at kDescKpCol = 23: the orientation disc in one
// 32-column MFMA window): a row is 12 dwords from x0 - 2, unaligned loads
// (the buffer base stays 4-aligned, the misalignment in the lane offset),
// so 5 rows a pass (lanes (rl, k), rl < 5) and 9 passes cover rows rl + 5 j;
// every row lane has j < 8, rows 40..42 (j = 8) only rl < 3.  One exec region
// for the nine loads and stores (the generic loop guards each with its own
// compare and exec save / restore: ~70 scalar instructions a wave), row
// offsets as scalar multiples of the pitch, LDS offsets as immediates.
// Stored XOR 0x80 (the int8 MFMAs' I - 128).  Needs x0 >= 2, x0 + 46 <= pitch.
constexpr int kDescCol0 = kDescKpCol - kDescR;   // 2: the patch column of the window's column 0
__device__ inline void stage_desc_patch(uint8_t *dst, const uint8_t *img, int pitch, int y0, int x0, int lane) {
    static_assert(kDescP == 43 && kDescPS == 48 && kDescCol0 == 2, "5 rows of 12 dwords a pass");
    pitch = __builtin_amdgcn_readfirstlane(pitch);
    const int xs = x0 - kDescCol0, xa = xs & ~3, sh = xs - xa;
    constexpr int nd = kDescPS / 4;
    const __amdgpu_buffer_rsrc_t src = wave_rsrc(img + (int64_t)y0 * pitch + xa);
    const int rl = lane / nd, k = lane - mul24u(rl, nd);
    const int voff = mul24u(rl, pitch) + 4 * k + sh;
    const int p5 = __builtin_amdgcn_readfirstlane(5 * pitch);
    typedef __attribute__((address_space(3))) uint32_t lds_u32;
    lds_u32 *d = (lds_u32 *)(dst + mul24u(rl, kDescPS) + 4 * k);
    if (rl < 5) {
        uint32_t v[9];
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = buf_ld32(src, voff, j * p5);
        const bool last = rl < 3;
        if (last) v[8] = buf_ld32(src, voff, 8 * p5);
#pragma unroll
        for (int j = 0; j < 8; ++j) d[j * 5 * kDescPS / 4] = v[j] ^ 0x80808080u;
        if (last) d[8 * 5 * kDescPS / 4] = v[8] ^ 0x80808080u;
    }
}

template <bool PIPE>
__global__ __launch_bounds__(kDescThreads, kDescWaves) void k_describe(DevPlan p, FrameBufs fb, int s0, int ns, int write_total,
                                                                   uint32_t gmagic) {
    __shared__ __align__(16) uint8_t lds[kDescW * kDescWaveStride];
    PHASE_START();
    const int tid = threadIdx.x, lane = tid & 63, wave = wave_id();
    int bx, b;
    xcd_block_2d(bx, b, gmagic);
    const int slot = s0 + bx * kDescW + wave;
    const bool in_range = slot < p.out_cap && bx * kDescW + wave < ns;
    // level of this slot (plan table) and the selected key: scalar loads
    const int l = in_range ? (int)p.slot_level[slot] : 0;
    // (32-bit index: the plan bounds max_batch * out_cap below 2^31, orbx_runtime.hip)
    const uint32_t key = in_range ? __builtin_amdgcn_readfirstlane(fb.sel[(uint32_t)(b * p.out_cap + slot)]) : 0u;
    // the frame's level counts: lane q < nlevels holds count q; the slot's
    // output offset is the prefix below its level (16-lane DPP scan)
    const int32_t *lc = fb.level_count + (uint32_t)(b * kMaxLevels);
    const int lq = lane & (kMaxLevels - 1);
    const int lcv = lc[lq];   // (every lane: a frame holds kMaxLevels counts)
    // the tables after the level counts: the scan below waits for the
    // counts alone (vector loads complete in order), not for the tables
    // this lane's 4 pattern pairs (pairs 64 g + lane, g = 0..3, as fp8 bytes
    // x0 y0 x1 y1 in word g), fetched first so the load overlaps the staging;
    // one buffer resource over each table, the loads at immediate offsets (the
    // compiler otherwise rebuilds a symbol's address, s_getpc + add + addc, per load)
    const __amdgpu_buffer_rsrc_t tab_rsrc = wave_rsrc(&c_desc);
    const long row_taps = __builtin_bit_cast(long, __builtin_amdgcn_raw_buffer_load_b64(tab_rsrc, 8 * lane, 4096, 0));
    const uint4 patq = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(tab_rsrc, 16 * lane, 3072, 0));
    // the moment products' operand tables (the same for every keypoint: the
    // patch is staged with the keypoint at a fixed column), ahead of the
    // key's chain of scalar loads and the staging, whose latency they hide under
    typedef uint64_t u64x2 __attribute__((ext_vector_type(2)));
    u64x2 mom[3];
    {
#pragma unroll
        for (int t = 0; t < 3; ++t)
            mom[t] = __builtin_bit_cast(u64x2, __builtin_amdgcn_raw_buffer_load_b128(tab_rsrc, 16 * lane + 1024 * t, 0, 0));
    }
    const int cq = lane < p.nlevels ? max(lcv, 0) : 0;
    static_assert(kMaxLevels == 16, "one DPP row");
    uint32_t scan = (uint32_t)cq;
    scan += dpp_or<kRowShr1>(0u, scan);
    scan += dpp_or<kRowShr2>(0u, scan);
    scan += dpp_or<kRowShr4>(0u, scan);
    scan += dpp_or<kRowShr8>(0u, scan);
    const int cl = __builtin_amdgcn_readlane(cq, l);
    const int off = __builtin_amdgcn_readlane((int)scan, l) - cl;
    if (write_total && bx == 0 && tid == 0) fb.nkps[b] = __builtin_amdgcn_readlane((int)scan, kMaxLevels - 1);
    const LevelArgs g = p.la[l];
    const int i = slot - g.out_off;
    const bool valid = in_range && i < cl;
    const int x = (int)(key & 0xFFF), y = (int)((key >> 12) & 0xFFF), score = (int)(key >> 24);

    uint8_t *lbase = lds + wave * kDescWaveStride;
    uint16_t *rowp = reinterpret_cast<uint16_t *>(lbase + kDescRowOff);
    // taps of getGaussianKernel(7, 2) x256 (checked against the plan on the host)
    constexpr int k0 = kGaussTaps[0], k1 = kGaussTaps[1], k2 = kGaussTaps[2], k3 = kGaussTaps[3];
    // column-pass taps as u16 pairs for v_dot2_u32_u16 over rows (r, r+1), (r+2, r+3), (r+4, r+5), (r+6, r+7)
    constexpr u16x2 kK01 = {(unsigned short)k0, (unsigned short)k1}, kK23 = {(unsigned short)k2, (unsigned short)k3},
                    kK21 = {(unsigned short)k2, (unsigned short)k1}, kK0z = {(unsigned short)k0, 0};
    // (the waves of a workgroup share nothing: no barrier to reach)
    if (!valid) return;
    int m01 = 0, m10 = 0;   // IC_Angle's moments, wave-uniform
    {

    // 1. stage the 43x43 unblurred neighbourhood at patch columns 2..44: dword
    //    loads when it lies inside the level, else byte loads with reflect-101
    //    at the borders
    int spitch;
    const uint8_t *img = level_ptr(p, fb, l, b, spitch);
    const int px0 = x - kDescR, py0 = y - kDescR;
    // (every term >= 0 <=> their OR is: one scalar compare instead of five compare / select / and)
    const bool inside = ((px0 - kDescCol0) | py0 | (g.w - 1 - kDescR - x) | (g.h - 1 - kDescR - y) |
                         (spitch - (px0 - kDescCol0 + kDescPS))) >= 0;
    if (inside) {
        stage_desc_patch(lbase, img, spitch, py0, px0, lane);
    } else {
        // near a level border: lane = patch column (its reflect-101 column fixed),
        // the rows in turn (the row's reflection is wave-uniform); columns
        // outside the window are not needed (multiplied by zero taps or feeding
        // unread outputs) and stay as they are
        const int c = min(max(lane, kDescCol0), kDescCol0 + kDescP - 1);
        const int xx = reflect101(px0 - kDescCol0 + c, g.w);
        const int sp = __builtin_amdgcn_readfirstlane(spitch);
        const bool col = lane >= kDescCol0 && lane < kDescCol0 + kDescP;
#pragma unroll 11
        for (int r = 0; r < kDescP; ++r) {
            const int yy = reflect101(py0 + r, g.h);
            const uint8_t v = img[(int64_t)yy * sp + xx];
            if (col) lbase[r * kDescPS + lane] = v ^ 0x80;
        }
    }
    wave_lds_fence();
    PHASE_MARK(1, 0);   // prologue + staging

    if constexpr (kStopDesc == 0 || kStopDesc >= 2) {
    // 2. IC_Angle's moments (ORBextractor.cc:77-104) and the horizontal pass of
    //    the 7x7 Gaussian, both as int8 MFMAs on the same pixel tiles.  The patch
    //    was staged as I - 128 (XOR 0x80); the moments over the disc do not see
    //    that bias (sum u = sum v = 0 over the symmetric disc) and the row pass's
    //    accumulator starts at 128 * sum(w) to undo it.
    {
        const int rl = lane & 15, q = lane >> 4;
        const uint8_t *bsrc = lbase + rl * kDescPS + 8 * q;
        uint64_t px[3][3];
#pragma unroll
        for (int rt = 0; rt < 3; ++rt)
#pragma unroll
            for (int ct = 0; ct < 3; ++ct)
                px[rt][ct] = *reinterpret_cast<const uint64_t *>(bsrc + 16 * rt * kDescPS + 16 * ct);
        // moments: A = the disc's pixels of the window tiles (rows 16 rt..,
        // columns 8..39), B = c_desc.mom's b; D[i][15] = sum of u I over row i,
        // D[i][12 + rt] = sum of I over row 16 rt + i, summed over the three
        // products (lane l: D[4 (l >> 4) + ii][l & 15])
        {
            static_assert(kDescKpCol - 15 == 8, "the disc's columns start the 8-aligned window");
            i32x4 acc = {0, 0, 0, 0};
#pragma unroll
            for (int rt = 0; rt < 3; ++rt) {
                const uint64_t pw = *reinterpret_cast<const uint64_t *>(bsrc + 16 * rt * kDescPS + 8);
                acc = __builtin_amdgcn_mfma_i32_16x16x32_i8((long)(pw & mom[rt].x), (long)mom[rt].y, acc, 0, 0, 0);
            }
            // m10: lane 15 of each row, S; m01: lanes 12..14, v-weighted rows
            // (v = 16 (j - 12) + 4 (l >> 4) + ii - 21), folded into lane 15
            const int j = rl;
            const int S = acc[0] + acc[1] + acc[2] + acc[3];
            const int T = acc[1] + 2 * acc[2] + 3 * acc[3];
            const bool rows = j >= 12 && j <= 14;
            int y = rows ? __mul24(16 * (j - 12) + 4 * q - 21, S) + T : 0;
            int x = S;
            asm volatile(
                "s_nop 1\n\t"
                "v_add_u32_dpp %0, %0, %0 row_shr:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
                "s_nop 1\n\t"
                "v_add_u32_dpp %0, %0, %0 row_shr:2 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
                "s_nop 1\n\t"
                "v_add_u32_dpp %0, %0, %0 row_bcast:15 row_mask:0xa bank_mask:0xf\n\t"
                "v_add_u32_dpp %1, %1, %1 row_bcast:15 row_mask:0xa bank_mask:0xf\n\t"
                "s_nop 1\n\t"
                "v_add_u32_dpp %0, %0, %0 row_bcast:31 row_mask:0xc bank_mask:0xf\n\t"
                "v_add_u32_dpp %1, %1, %1 row_bcast:31 row_mask:0xc bank_mask:0xf\n\t"
                "s_nop 1"
                : "+v"(y), "+v"(x));
            m01 = __builtin_amdgcn_readlane(y, 63);
            m10 = __builtin_amdgcn_readlane(x, 63);
        }
        PHASE_MARK(1, 1);   // moments
        // row pass: nine 16 x 16 output tiles (rows 16 rt.., patch columns
        // 16 ct..; window column = patch column - o), D = P T: A operand, lane
        // l holds P[16 rt + (l & 15)][16 ct + 8 (l >> 4) + 0..7] - 128 (one
        // ds_read_b64); B = the Toeplitz taps.  D's lane l holds rows
        // 16 rt + 4 (l >> 4) + 0..3 of output column 16 ct + (l & 15): one
        // 8-byte store into the column-major buffer.  Only columns < 40 and
        // rows < 44 are stored (row 43 is padding).
        const i32x4 bias = {128 * 257, 128 * 257, 128 * 257, 128 * 257};
        static_assert(kGaussTaps[0] + kGaussTaps[1] + kGaussTaps[2] + kGaussTaps[3] + kGaussTaps[4] +
                          kGaussTaps[5] + kGaussTaps[6] == 257, "bias = 128 * sum of the taps");
        // Every lane stores (no exec regions): the outputs outside the buffer
        // land where a later store of the same wave rewrites them (LDS stores
        // of a wave complete in order; compiler barriers keep that order):
        //  - rows 44..47 (rt = 2, q = 3) are rows 0..3 of the next column,
        //    rewritten by the rt = 0 tiles, stored last (the last column's
        //    go to the buffer's 8 spare bytes);
        //  - columns 40..47 (ct = 2, rl >= 8) are sent to columns 0..7 of the
        //    same rows, rewritten by the ct = 0 tile stored after it.
        static_assert(kRowCols == 40 && kColS == 44, "the spill targets above");
        uint16_t *dst = rowp + rl * kColS + 4 * q;
        uint16_t *dst2 = rowp + (rl < kRowCols - 32 ? rl + 32 : rl - 8) * kColS + 4 * q;   // tile ct = 2
        auto store = [&](int rt, int ct) {
            const i32x4 d = __builtin_amdgcn_mfma_i32_16x16x32_i8((long)px[rt][ct], row_taps, bias, 0, 0, 0);
            uint2 w;
            w.x = __builtin_amdgcn_perm((uint32_t)d[1], (uint32_t)d[0], 0x05040100u);   // (d0, d1) as u16 halves
            w.y = __builtin_amdgcn_perm((uint32_t)d[3], (uint32_t)d[2], 0x05040100u);
            *reinterpret_cast<uint2 *>((ct == 2 ? dst2 : dst + 16 * ct * kColS) + 16 * rt) = w;
            asm volatile("" ::: "memory");
        };
#pragma unroll
        for (int rt = 2; rt >= 0; --rt) {
            store(rt, 2);
            store(rt, 0);
            store(rt, 1);
        }
    }
    PHASE_MARK(1, 2);   // row pass
    }   // kStopDesc
    }
    // The orientation (fastAtan2) and its sincosf: wave-uniform chains of ~90
    // VALU that every wave issues for its own keypoint.  One wave evaluating its
    // workgroup's orientations between two barriers issued a quarter of that
    // per keypoint and measured slower: the chain advances one instruction per
    // turn of its SIMD's waves, and the workgroup's other waves waited it out
    // (profiles/r07_ab_describe.txt).
    const float angle = fast_atan2_deg((float)m01, (float)m10);
    float sa, ca;
    glibc_sincosf(__fmul_rn(angle, (float)(3.14159265358979323846 / 180.f)), &sa, &ca);
    PHASE_MARK(1, 5);   // orientation
    const int64_t kp_index = (int64_t)b * p.max_kps + off + i;
    // the keypoint record (the matchers downstream index their grids with it)
    auto write_record = [&]() {
        if (lane == 0) {
            orbx_keypoint kp;
            float fx = (float)x, fy = (float)y;
            if (l != 0) { fx = __fmul_rn(fx, g.scale); fy = __fmul_rn(fy, g.scale); }
            kp.x = fx;
            kp.y = fy;
            kp.size = g.patch_size;
            kp.angle = angle;
            kp.response = (float)score;
            kp.octave = l;
            kp.class_id = -1;
            fb.kps[kp_index] = kp;
        }
    };
    if constexpr (kStopDesc != 0 && kStopDesc < 4) {
        write_record();
        return;
    }

    // 4. computeOrbDescriptor (ORBextractor.cc:106-147) on the blurred level:
    //    each sample's blurred value is the column pass evaluated at that pixel
    //    from the row-pass buffer, with OpenCV 3.2's per-column rounding
    //    (half-even below w & ~3, else half-up).
    const int xs = g.w & ~3;
    // whole sample window left of w & ~3 (almost every keypoint): half-even
    // rounding everywhere, (s + 0x7FFF + bit16) >> 16, no per-column test
    const bool all_even = x + kBlurR < xs;
    // all 8 of the lane's samples: offsets, then every column-pass read in
    // flight at once, then the rounding
    // A sample at window offset (r, c) reads column c + kBlurR + kDescCol0, rows
    // r + kBlurR .. +6 of the column-major buffer: byte offset
    // 2 kColS (c + kBlurR + kDescCol0) + 2 (r + kBlurR), from the cvRound'ed float
    // bits (0x4B400000 + n, below) as one 24-bit multiply-add and one
    // shift-add; the constant folds the bias bits away (mod 2^32).  The read
    // is the four dwords from the one holding row r down (two ds_read2_b32;
    // unaligned ds_read_b128 measured 470 stall cycles a wave), and an odd
    // row's pairs are realigned by 16 bits (v_alignbit by a per-lane shift).
    const uint32_t kOff = (uint32_t)(kDescRowOff + 2 * kColS * (kBlurR + kDescCol0) + 2 * kBlurR) -
                          (uint32_t)(2 * kColS) * 0x400000u - 2u * 0x4B400000u;
    static_assert((kDescRowOff & 3) == 0 && (kColS & 1) == 0, "dword-aligned column starts");
    typedef uint32_t u32x4a __attribute__((ext_vector_type(4), aligned(4)));
    typedef __attribute__((address_space(3))) const u32x4a lds_u32x4a;
    // the LDS address of the wave's buffer folded into the constant: the
    // address is then one v_lshl_add and one v_mad_u32_u24 from the bits
    const uint32_t kOffL = __builtin_amdgcn_readfirstlane(kOff + (uint32_t)(uintptr_t)(const lds_u8 *)lbase);
    int sums[8], cbs[8];
    typedef float f32x2 __attribute__((ext_vector_type(2)));
    // cvRound by the 1.5 * 2^23 bias: the float add rounds to the nearest
    // integer, ties to even, and the bits are then 0x4B400000 + n (|n| < 2^22)
    constexpr float kRndBias = 12582912.f;
    const f32x2 sc = {sa, ca}, rnd2 = {kRndBias, kRndBias};
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const uint32_t pw = (k >> 1) == 0 ? patq.x : (k >> 1) == 1 ? patq.y : (k >> 1) == 2 ? patq.z : patq.w;
        // (rb, cb) side by side as packed f32 pairs (v_pk_mul / v_pk_add:
        // the same IEEE products and sums, two per instruction):
        //   rb = (px sa + py ca) + bias,  cb = (px ca - py sa) + bias
        // (written out: the compiler's own packing negates and moves pairs around;
        // the same eight steps as unpacked VOP2 f32 ops on VGPR operands took
        // fewer issue cycles and more instructions, time neutral,
        // profiles/r06_ab_desc_f32.txt)
        const f32x2 pxy = (k & 1) ? __builtin_amdgcn_cvt_pk_f32_fp8((int)pw, true)      // (x, y) of point k
                                  : __builtin_amdgcn_cvt_pk_f32_fp8((int)pw, false);
        f32x2 rc;
        f32x2 py2;
        asm("v_pk_mul_f32 %0, %2, %3 op_sel_hi:[0,1]\n\t"               // (px sa, px ca)
            "v_pk_mul_f32 %1, %2, %3 op_sel:[1,1] op_sel_hi:[1,0]\n\t"  // (py ca, py sa)
            "v_pk_add_f32 %0, %0, %1 neg_hi:[0,1]\n\t"                  // (px sa + py ca, px ca - py sa)
            "v_pk_add_f32 %0, %0, %4"                                   // + (bias, bias)
            : "=&v"(rc), "=&v"(py2)
            : "v"(pxy), "v"(sc), "s"(rnd2));
        const uint32_t rb = __float_as_uint(rc.x), cb = __float_as_uint(rc.y);
        cbs[k] = (int)cb;
        // (__umul24 reads the low 24 bits of cb: 0x400000 + c, c in [-18, 18])
        uint32_t t, off;
        asm("v_lshl_add_u32 %0, %1, 1, %2" : "=v"(t) : "v"(rb), "s"(kOffL));
        asm("v_mad_u32_u24 %0, %1, %2, %3" : "=v"(off) : "v"(cb), "s"(2u * kColS), "v"(t));
        const u32x4a v = *reinterpret_cast<lds_u32x4a *>((uintptr_t)(off & ~3u));
        // odd row (the low bit of rb): shift 16; v_alignbit reads its shift's low 5 bits
        const uint32_t sh = rb << 4;
        // k0 R0 + k1 R1 + k2 R2 + k3 R3 + k2 R4 + k1 R5 + k0 R6 as four u16-pair dot products
        const uint32_t e0 = __builtin_amdgcn_alignbit(v.y, v.x, sh), e1 = __builtin_amdgcn_alignbit(v.z, v.y, sh),
                       e2 = __builtin_amdgcn_alignbit(v.w, v.z, sh), e3 = __builtin_amdgcn_alignbit(v.w, v.w, sh);
        sums[k] = (int)__builtin_amdgcn_udot2(
            as_u16x2(e0), kK01,
            __builtin_amdgcn_udot2(as_u16x2(e1), kK23,
                                   __builtin_amdgcn_udot2(as_u16x2(e2), kK21,
                                                          __builtin_amdgcn_udot2(as_u16x2(e3), kK0z, 0u, false),
                                                          false),
                                   false),
            false);
    }
    PHASE_MARK(1, 3);   // sincos + sample offsets + column pass
    if constexpr (kStopDesc == 4) {   // keep the column pass: its sums reach LDS
        int acc = 0;
#pragma unroll
        for (int k = 0; k < 8; ++k) acc ^= sums[k] + cbs[k];
        if (acc == 0x7FFFFFFF) lbase[0] = 1;
        write_record();
        return;
    }
    int val[8];
    if (all_even) {
#pragma unroll
        for (int k = 0; k < 8; ++k) val[k] = min((sums[k] + 0x7FFF + ((sums[k] >> 16) & 1)) >> 16, 255);
    } else {
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int sum = sums[k];
            int qv;
            if (x + (cbs[k] - 0x4B400000) < xs) {
                qv = sum >> 16;
                const int rem = sum & 0xFFFF;
                qv += (rem > 0x8000) | ((rem == 0x8000) & (qv & 1));
            } else {
                qv = (sum + (1 << 15)) >> 16;
            }
            val[k] = min(qv, 255);
        }
    }
    uint64_t m[4];
#pragma unroll
    for (int grp = 0; grp < 4; ++grp) m[grp] = lanes_lt(val[2 * grp], val[2 * grp + 1]);
    if (lane == 0) {
        ulonglong2 *dout = reinterpret_cast<ulonglong2 *>(fb.desc + kp_index * 32);
        dout[0] = make_ulonglong2(m[0], m[1]);
        dout[1] = make_ulonglong2(m[2], m[3]);
    }
    write_record();
    PHASE_MARK(1, 4);   // rounding + ballots + records
}

__global__ void k_trig(const float *in, float *so, float *co, int n, const float *ay, const float *ax,
                       float *at, int m) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) glibc_sincosf(in[i], &so[i], &co[i]);
    if (i < m) at[i] = fast_atan2_deg(ay[i], ax[i]);
}

}  // namespace

hipError_t launch_blur(const DevPlan &p, const FrameBufs &fb, int B, hipStream_t st) {
    hipLaunchKernelGGL(k_blur, dim3(p.nblur_tiles, B), dim3(kThreads), 0, st, p, fb);
    return hipGetLastError();
}

hipError_t launch_describe(const DevPlan &p, const FrameBufs &fb, int B, hipStream_t st) {
    const uint32_t gx = (p.out_cap + kDescW - 1) / kDescW;
    hipLaunchKernelGGL(k_describe<false>, dim3(gx, B), dim3(kDescThreads), 0, st, p, fb, 0, p.out_cap, 1,
                       grid_magic(gx, B));
    return hipGetLastError();
}

// Levels [l, l_end)'s keypoints; the launch with the last level also writes each
// frame's keypoint total (every level's count is final by then).
hipError_t launch_describe_level(const DevPlan &p, const Plan &hp, const FrameBufs &fb, int B, hipStream_t st, int l,
                                 int l_end) {
    const int s0 = hp.lv[l].out_off, ns = hp.lv[l_end - 1].out_off + hp.lv[l_end - 1].out_cap - s0;
    const uint32_t gx = (ns + kDescW - 1) / kDescW;
    hipLaunchKernelGGL(k_describe<true>, dim3(gx, B), dim3(kDescThreads), 0, st, p, fb, s0, ns,
                       l_end == hp.nlevels ? 1 : 0, grid_magic(gx, B));
    return hipGetLastError();
}

hipError_t launch_trig_check(const float *in, float *s, float *c, float *atan_out, const float *ay,
                             const float *ax, int n, int m, hipStream_t st) {
    const int total = n > m ? n : m;
    if (total <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_trig, dim3((total + 255) / 256), dim3(256), 0, st, in, s, c, n, ay, ax, atan_out, m);
    return hipGetLastError();
}

}  // namespace orbx
