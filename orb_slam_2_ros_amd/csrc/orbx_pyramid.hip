// orbx_pyramid.hip -- the image pyramid of the ORB extractor on gfx950.
//
// Stage                       reference (wjjcdy/orb_slam_2_ros)
//   k_resize   (x7 levels)    ComputePyramid, ORBextractor.cc:1152-1185 (+cv::resize)
// as the block kernel k_resize, the wave-tile kernels k_resize_w / k_resize_d
// and the one-launch region pyramid k_pyramid_rgn, with their launchers and
// host-side planners.  Integer / byte work bound by HBM and VALU issue.
#include "orbx_extract_util.h"

namespace orbx {

namespace {

// ===========================================================================
// K1: bilinear level l from level l-1 (cv::resize INTER_LINEAR 8U, OpenCV 3.2
// fixed point; SSE2 vertical rounding on the leading columns, scalar tail).
// Block = 256 x 8 output pixels; the source window it needs (<= kResRows x
// kResCols bytes, checked on the host) is staged in LDS by coalesced loads.
// Thread = 4 consecutive columns x 2 rows, one u32 store per row.
// ===========================================================================
constexpr int kResTW = 256, kResTH = 16, kResRows = 32, kResCols = 544;
constexpr int kResRowsPerThread = kResTH / 4;

__global__ __launch_bounds__(kThreads) void k_resize(DevPlan p, FrameBufs fb, int l) {
    __shared__ uint8_t win[kResRows * kResCols];
    const LevelGeom g = p.lv[l];
    const LevelGeom gs = p.lv[l - 1];
    const int tid = threadIdx.x;
    const int L = xcd_logical_block((blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x,
                                    gridDim.x * gridDim.y * gridDim.z);
    const int bxy = L % (gridDim.x * gridDim.y), b = L / (gridDim.x * gridDim.y);
    const int x0 = (bxy % gridDim.x) * kResTW, y0 = (bxy / gridDim.x) * kResTH;
    const ResizeTap *xt = p.xtaps + g.xtab_off;
    const ResizeTap *yt = p.ytaps + g.ytab_off;
    // this thread's taps: 4 columns x kResRowsPerThread rows, fetched before the
    // window so their latency overlaps the staging loads
    const int xb = x0 + 4 * (tid & 63);
    const int yb = y0 + kResRowsPerThread * (tid >> 6);
    ResizeTap tx[4], ty[kResRowsPerThread];
#pragma unroll
    for (int k = 0; k < 4; ++k) tx[k] = xt[min(xb + k, g.w - 1)];
#pragma unroll
    for (int k = 0; k < kResRowsPerThread; ++k) ty[k] = yt[min(yb + k, g.h - 1)];
    const int xl = min(x0 + kResTW, g.w) - 1, yl = min(y0 + kResTH, g.h) - 1;
    const int c_lo = xt[x0].src, c_hi = min((int)xt[xl].src + 1, gs.w - 1);
    const int r_lo = min(max((int)yt[y0].src, 0), gs.h - 1);
    const int r_hi = min(max((int)yt[yl].src + 1, 0), gs.h - 1);
    const int nc = c_hi - c_lo + 1, nr = r_hi - r_lo + 1;
    int spitch;
    const uint8_t *src = level_ptr(p, fb, gs, l - 1, b, spitch);
    // each wave stages a quarter of the window's rows (aligned dword loads)
    const int wv = tid >> 6;
    const int ra = (nr * wv) >> 2, rb = (nr * (wv + 1)) >> 2;
    int o = c_lo & 3;
    if (rb > ra) o = wave_stage_rect(win + ra * kResCols, kResCols, src, spitch, r_lo + ra, c_lo, rb - ra, nc, tid & 63);
    __syncthreads();
    if (xb >= g.w) return;
    uint8_t *dst = fb.pyr + (int64_t)b * p.pyr_bytes + g.pyr_off;
    // An opaque 1: stops the load vectorizer from fusing the tap pair S[sx],
    // S[sx+1] into one unaligned ds_read_u16 (LDS unaligned-access stalls).
    int one = 1;
    asm volatile("" : "+s"(one));
#pragma unroll
    for (int rr = 0; rr < kResRowsPerThread; ++rr) {
        const int y = yb + rr;
        if (y >= g.h) break;
        const lds_u8 *S0 = (const lds_u8 *)(win + mul24u(min(max((int)ty[rr].src, 0), gs.h - 1) - r_lo, kResCols) + o - c_lo);
        const lds_u8 *S1 = (const lds_u8 *)(win + mul24u(min(max((int)ty[rr].src + 1, 0), gs.h - 1) - r_lo, kResCols) + o - c_lo);
        const int b0 = ty[rr].a0, b1 = ty[rr].a1;
        uint32_t packed = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            // Branch-free: tail columns carry coefficients (2048, 0) (orbx_plan.h);
            // every product fits 24-bit operands (S <= 255, a <= 2048, h < 2^20).
            const int sx = tx[k].src, sx1 = sx + one;
            const int h0 = mul24u(S0[sx], tx[k].a0) + mul24u(S0[sx1], tx[k].a1);
            const int h1 = mul24u(S1[sx], tx[k].a0) + mul24u(S1[sx1], tx[k].a1);
            // SSE2 columns: _mm_packs_epi32(h>>4); _mm_mulhi_epi16; _mm_adds_epi16; +2; >>2; packus
            const int v_simd = ((mul24u(h0 >> 4, b0) >> 16) + (mul24u(h1 >> 4, b1) >> 16) + 2) >> 2;
            // scalar tail: FixedPtCast<int, uchar, 22>
            const int v_tail = (mul24u(h0, b0) + mul24u(h1, b1) + (1 << 21)) >> 22;
            const int v = (tx[k].mode & 2) ? v_simd : v_tail;
            packed |= (uint32_t)min(max(v, 0), 255) << (8 * k);
        }
        *reinterpret_cast<uint32_t *>(dst + mul24u(y, g.pitch) + xb) = packed;
    }
}

// ===========================================================================
// K1 (wave tiles): the same resize with every wave independent.  A wave owns
// a 4*twg x (64/twg)*kResizeK output tile (ResizeWave, chosen per level so
// narrow levels waste few lanes), stages the source window it needs in its
// own LDS slice and writes 4 columns x kResizeK rows per lane.  The window
// bounds come from the same double/float arithmetic as the tap tables, so the
// staging loads and the tap loads go out together.  Per source row a lane
// reads 3 dwords, realigns them, gathers each column's pixel pair (S[sx],
// S[sx+1]) with one v_perm and applies the horizontal taps with one
// v_dot2_u32_u16; the vertical pass is OpenCV's fixed point as above.
// ===========================================================================
typedef unsigned short u16x2_t __attribute__((ext_vector_type(2)));

__host__ __device__ inline int resize_src_raw(int d, double scale) {
#ifdef __HIP_DEVICE_COMPILE__
    const float f = __double2float_rn(__dsub_rn(__dmul_rn(__dadd_rn((double)d, 0.5), scale), 0.5));
    return (int)floorf(f);
#else
    const float f = (float)((d + 0.5) * scale - 0.5);
    return floor_i(f);
#endif
}

// The SSE2 columns' vertical pass of 4 columns, packed into one dword:
// ((h0 >> 4) b0 >> 16) + ((h1 >> 4) b1 >> 16), + 2, >> 2 (each sum <= 1022),
// the >> 16 as the high half of (h & ~15) x (b << 12) (24-bit operands, bb =
// b << 12).  Two sums share a dword (s0 + s1 << 16 + 0x20002, no carry between
// the halves), one shift rounds both, one v_perm packs the four bytes.
__device__ inline uint32_t resize_vpass_simd(const uint32_t h0[4], const uint32_t h1[4], uint32_t bb0, uint32_t bb1) {
    uint32_t sm[4];
#pragma unroll
    for (int k = 0; k < 4; ++k)
        sm[k] = (uint32_t)(((uint64_t)(h0[k] & 0xFFFF0u) * bb0) >> 32) + (uint32_t)(((uint64_t)(h1[k] & 0xFFFF0u) * bb1) >> 32);
    const uint32_t p01 = ((sm[1] << 16) + sm[0] + 0x00020002u) >> 2;
    const uint32_t p23 = ((sm[3] << 16) + sm[2] + 0x00020002u) >> 2;
    return __builtin_amdgcn_perm(p23, p01, 0x06040200u);
}

// One wave tile (ResizeWave) of level l of frame b; `win` is the wave's LDS
// slice (a.win_bytes).
template <int NB>
__device__ inline void resize_tile(const DevPlan &p, const FrameBufs &fb, int l, const ResizeWave &a, int b, int tile,
                                   int lane, uint8_t *win) {
    wave_lds_fence();   // the slice's previous window is consumed
    const int ty = tile / a.ntx, tx = tile - ty * a.ntx;
    const LevelArgs g = p.la[l], gs = p.la[l - 1];
    const int twg = a.twg, lr = lane >> a.twg_shift, lg = lane & (twg - 1);
    const int TH = (64 >> a.twg_shift) * kResizeK;
    const int x0 = tx * 4 * twg, y0 = ty * TH;
    const int xb = x0 + 4 * lg, yb = y0 + lr * kResizeK;
    // taps of this lane's 4 columns and kResizeK rows (independent of the window loads)
    // (buffer loads: 32-bit lane offsets from the wave's table bases)
    static_assert(sizeof(ResizeTap) == 8, "one dwordx2 a tap");
    const __amdgpu_buffer_rsrc_t xt = wave_rsrc(p.xtaps + a.xtab_off), yt = wave_rsrc(p.ytaps + a.ytab_off);
    ResizeTap txk[4], tyk[kResizeK];
#pragma unroll
    for (int k = 0; k < 4; ++k)
        txk[k] = __builtin_bit_cast(ResizeTap, __builtin_amdgcn_raw_buffer_load_b64(xt, 8 * min(xb + k, g.w - 1), 0, 0));
#pragma unroll
    for (int k = 0; k < kResizeK; ++k)
        tyk[k] = __builtin_bit_cast(ResizeTap, __builtin_amdgcn_raw_buffer_load_b64(yt, 8 * min(yb + k, g.h - 1), 0, 0));
    // the source window: columns [c_lo, c_hi], rows [r_lo, r_hi] (as the tables)
    const int xl = min(x0 + 4 * twg, g.w) - 1, yl = min(y0 + TH, g.h) - 1;
    const int c_lo = min(max(resize_src_raw(x0, a.sx), 0), gs.w - 1);
    const int c_hi = min(max(resize_src_raw(xl, a.sx), 0) + 1, gs.w - 1);
    const int r_lo = min(max(resize_src_raw(y0, a.sy), 0), gs.h - 1);
    const int r_hi = min(max(resize_src_raw(yl, a.sy) + 1, 0), gs.h - 1);
    int spitch;
    const uint8_t *src = level_ptr(p, fb, l - 1, b, spitch);
    wave_stage_rows<NB, false>(win, a.win_stride, src, spitch, r_lo, c_lo, r_hi - r_lo + 1, c_hi - c_lo + 1, lane);
    // per-lane column constants: dword of the first source pixel, realignment,
    // and the v_perm selectors of the 4 pixel pairs (S[sx_k], S[sx_k + 1])
    const int rel0 = txk[0].src - (c_lo & ~3);
    const int q4 = (rel0 >> 2) * 4, o = rel0 & 3;
    uint32_t sel[4], coef[4];
    bool simd_all = true;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const uint32_t r = (uint32_t)(txk[k].src - txk[0].src);
        sel[k] = r | 0x0C00u | ((r + 1) << 16) | 0x0C000000u;
        coef[k] = (uint32_t)(uint16_t)txk[k].a0 | ((uint32_t)(uint16_t)txk[k].a1 << 16);
        simd_all &= (txk[k].mode & 2) != 0;
    }
    wave_lds_fence();
    if (xb >= g.w) return;
    // (buffer stores: a 32-bit lane offset from the wave's level base, no
    // 64-bit address arithmetic per row)
    const __amdgpu_buffer_rsrc_t dst = wave_rsrc(fb.pyr + (int64_t)b * p.pyr_bytes + g.pyr_off);
    auto hrow = [&](int row, uint32_t h[4]) {
        const uint32_t *ap = reinterpret_cast<const uint32_t *>(win + mul24u(row - r_lo, a.win_stride) + q4);
        const uint32_t d0 = ap[0], d1 = ap[1], d2 = ap[2];
        const uint32_t w0 = __builtin_amdgcn_alignbyte(d1, d0, o), w1 = __builtin_amdgcn_alignbyte(d2, d1, o);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint32_t pr = __builtin_amdgcn_perm(w1, w0, sel[k]);
            h[k] = __builtin_amdgcn_udot2(__builtin_bit_cast(u16x2_t, pr), __builtin_bit_cast(u16x2_t, coef[k]), 0u,
                                          false);
        }
    };
    // the horizontal pass of source row `prow` from the previous output row:
    // the next row's first source row is usually the previous one's second
    uint32_t hp[4] = {0u, 0u, 0u, 0u};
    int prow = -1;
#pragma unroll
    for (int j = 0; j < kResizeK; ++j) {
        const int y = yb + j;
        if (y >= g.h) break;
        const int s0 = min(max((int)tyk[j].src, 0), gs.h - 1), s1 = min(max((int)tyk[j].src + 1, 0), gs.h - 1);
        const int b0 = tyk[j].a0, b1 = tyk[j].a1;
        uint32_t h0[4], h1[4];
        if (s0 == prow) {
#pragma unroll
            for (int k = 0; k < 4; ++k) h0[k] = hp[k];
        } else {
            hrow(s0, h0);
        }
        hrow(s1, h1);
        prow = s1;
#pragma unroll
        for (int k = 0; k < 4; ++k) hp[k] = h1[k];
        // SSE2 columns: _mm_packs_epi32(h>>4); _mm_mulhi_epi16; _mm_adds_epi16; +2; >>2
        // (h <= 255 * 2048: no saturation, result <= 255); the last < 16 columns
        // are the scalar tail FixedPtCast<int, uchar, 22>
        uint32_t packed = 0;
        if (simd_all) {
            // ((h >> 4) * b) >> 16 as the high half of a 24 x 24-bit product:
            // (h & ~15) * (b << 12) = ((h >> 4) * b) << 16, both operands < 2^24
            const uint32_t bb0 = ((uint32_t)b0 & 0xFFFu) << 12, bb1 = ((uint32_t)b1 & 0xFFFu) << 12;   // (b <= 2048)
            packed = resize_vpass_simd(h0, h1, bb0, bb1);
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const uint32_t v = (txk[k].mode & 2)
                                       ? ((mul24u(h0[k] >> 4, b0) >> 16) + (mul24u(h1[k] >> 4, b1) >> 16) + 2) >> 2
                                       : (mul24u(h0[k], b0) + mul24u(h1[k], b1) + (1 << 21)) >> 22;
                packed |= v << (8 * k);
            }
        }
        __builtin_amdgcn_raw_buffer_store_b32(packed, dst, mul24u(y, g.pitch) + xb, 0, 0);
    }
}

template <int NB>
__global__ __launch_bounds__(kThreads) void k_resize_w(DevPlan p, FrameBufs fb, int l, ResizeWave a, int B) {
    extern __shared__ __align__(16) uint8_t lds[];
    const int wave = wave_id(), lane = threadIdx.x & 63;
    const int L = xcd_logical_block(blockIdx.x, gridDim.x);
    const int t = L * 4 + wave;
    if (t >= a.ntiles * B) return;
    const int b = t / a.ntiles;
    resize_tile<NB>(p, fb, l, a, b, t - b * a.ntiles, lane, lds + wave * a.win_bytes);
}

// ===========================================================================
// K1 (direct wave tiles): the same tiles and arithmetic without the LDS
// window.  A lane's 4 columns read source bytes sx_0 .. sx_3 + 1, at most 7
// apart (plan_resize_waves), so each source row is ONE dword-aligned 12-byte
// buffer load (8 bytes from cs = min(sx_0, w_src - 8) after v_alignbyte; a
// pair byte past them, only the last column's S[sx + 1] whose coefficient is
// 0 there, is selected as zero).  The lane's column constants (load column,
// realignment, v_perm selectors, coefficients) and its rows' clamped source
// rows and vertical coefficients are host tables (ResizeCol, ResizeRow), so
// the kernel does no tap arithmetic.  The window staging (half of
// resize_tile's VALU: predicated loads and LDS stores a row) goes; L1/L2
// serve the rows the lanes share.  Unaligned 8-byte loads instead of the
// 12-byte aligned ones measured slower (resize 1.80 vs 1.52 ms a step,
// profiles/r05_ab_resize_direct.txt).
// ===========================================================================
__device__ inline void resize_tile_direct(const DevPlan &p, const FrameBufs &fb, int l, const ResizeWave &a, int b,
                                          int tile, int lane) {
    const int ty = tile / a.ntx, tx = tile - ty * a.ntx;
    const LevelArgs g = p.la[l], gs = p.la[l - 1];
    const int twg = a.twg, lr = lane >> a.twg_shift, lg = lane & (twg - 1);
    const int TH = (64 >> a.twg_shift) * kResizeK;
    const int x0 = tx * 4 * twg, y0 = ty * TH;
    const int xb = x0 + 4 * lg, yb = y0 + lr * kResizeK;
    if (xb >= g.w) return;
    // this lane's column group and rows (host tables: no per-lane tap arithmetic)
    const __amdgpu_buffer_rsrc_t ct = wave_rsrc(p.rcols + a.col_off), rt = wave_rsrc(p.rrows + a.ytab_off);
    typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
    typedef uint32_t u32x3 __attribute__((ext_vector_type(3)));
    const u32x3 cg0 = __builtin_amdgcn_raw_buffer_load_b96(ct, 12 * xb, 0, 0);     // c, o, smask
    const u32x4 cg1 = __builtin_amdgcn_raw_buffer_load_b128(ct, 12 * xb + 16, 0, 0);   // sel
    const u32x4 cg2 = __builtin_amdgcn_raw_buffer_load_b128(ct, 12 * xb + 32, 0, 0);   // coef
    typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
    u32x2 rw[kResizeK];
#pragma unroll
    for (int j = 0; j < kResizeK; ++j) rw[j] = __builtin_amdgcn_raw_buffer_load_b64(rt, 8 * min(yb + j, g.h - 1), 0, 0);
    int spitch;
    __amdgpu_buffer_rsrc_t src = wave_rsrc(level_ptr(p, fb, l - 1, b, spitch));
    spitch = __builtin_amdgcn_readfirstlane(spitch);
    if (l == 1) {
        // level 0 is the caller's image: the buffer's range ends at its last
        // row's last dword (a dword never crosses a page), so the dword loads
        // of the last row's right end cannot fault
        const uint64_t a0 = reinterpret_cast<uint64_t>(level_ptr(p, fb, 0, b, spitch));
        const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)a0), hi = __builtin_amdgcn_readfirstlane((uint32_t)(a0 >> 32));
        src = __builtin_amdgcn_make_buffer_rsrc(reinterpret_cast<void *>(((uint64_t)hi << 32) | lo), (short)0,
                                                ((gs.h - 1) * spitch + gs.w + 3) & ~3, 0x00020000);
    }
    const int c = (int)cg0.x, o = (int)cg0.y;
    const uint32_t smask = cg0.z;
    const uint32_t sel[4] = {cg1.x, cg1.y, cg1.z, cg1.w}, coef[4] = {cg2.x, cg2.y, cg2.z, cg2.w};
    // every source row the lane needs, loaded before any is used; a row shared
    // with the previous output row is not loaded again (at the 1.2 factor 2 of
    // 3 output rows reuse one)
    u32x3 d0[kResizeK], d1[kResizeK];
    int s1p = -1;
#pragma unroll
    for (int j = 0; j < kResizeK; ++j) {
        const int s0 = (int)(rw[j].x & 0xFFFFu), s1 = (int)(rw[j].x >> 16);
        if (s0 != s1p) d0[j] = __builtin_amdgcn_raw_buffer_load_b96(src, mul24u(s0, spitch) + c, 0, 0);
        d1[j] = __builtin_amdgcn_raw_buffer_load_b96(src, mul24u(s1, spitch) + c, 0, 0);
        s1p = s1;
    }
    const __amdgpu_buffer_rsrc_t dst = wave_rsrc(fb.pyr + (int64_t)b * p.pyr_bytes + g.pyr_off);
    auto hrow = [&](u32x3 d, uint32_t h[4]) {
        const uint32_t w0 = __builtin_amdgcn_alignbyte(d.y, d.x, o), w1 = __builtin_amdgcn_alignbyte(d.z, d.y, o);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint32_t pr = __builtin_amdgcn_perm(w1, w0, sel[k]);
            h[k] = __builtin_amdgcn_udot2(__builtin_bit_cast(u16x2_t, pr), __builtin_bit_cast(u16x2_t, coef[k]), 0u,
                                          false);
        }
    };
    uint32_t hp[4] = {0u, 0u, 0u, 0u};
    int prow = -1;
#pragma unroll
    for (int j = 0; j < kResizeK; ++j) {
        const int y = yb + j;
        if (y >= g.h) break;
        const int s0 = (int)(rw[j].x & 0xFFFFu), s1 = (int)(rw[j].x >> 16);
        const uint32_t bb0 = (rw[j].y & 0xFFFFu) << 12, bb1 = (rw[j].y >> 16) << 12;
        uint32_t h0[4], h1[4];
        if (s0 == prow) {
#pragma unroll
            for (int k = 0; k < 4; ++k) h0[k] = hp[k];
        } else {
            hrow(d0[j], h0);
        }
        hrow(d1[j], h1);
        prow = s1;
#pragma unroll
        for (int k = 0; k < 4; ++k) hp[k] = h1[k];
        uint32_t packed = 0;
        if (smask == 0xFu) {
            packed = resize_vpass_simd(h0, h1, bb0, bb1);
        } else {
            const uint32_t b0 = bb0 >> 12, b1 = bb1 >> 12;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const uint32_t v = (smask >> k & 1u)
                                       ? ((mul24u(h0[k] >> 4, b0) >> 16) + (mul24u(h1[k] >> 4, b1) >> 16) + 2) >> 2
                                       : (mul24u(h0[k], b0) + mul24u(h1[k], b1) + (1 << 21)) >> 22;
                packed |= v << (8 * k);
            }
        }
        __builtin_amdgcn_raw_buffer_store_b32(packed, dst, mul24u(y, g.pitch) + xb, 0, 0);
    }
}

// A phase-uniform tile row (ResizeTileRow, plan_resize_waves): every lane
// group's kResizeK rows lie inside the level, no source row is clamped and the
// groups' source rows advance by one shared sequence, so the row schedule is
// the wave's and not the lane's.  A lane keeps two bases (its group's first
// source row and its first output row, one v_mad each); every row's source and
// store offsets are scalar multiples of the pitches in the buffer
// instructions' scalar offset, the reuse of the previous row's horizontal
// pass is a scalar branch on the shared pattern, there is no y < h test, and
// the row records are read for their coefficients alone.
// Scalar branches and not one body per pattern: the patterns of a plan are
// few at exactly 1.2 but drift with the phase at every other ratio (333 ->
// 278), and a branch costs two SALU a row beside ~30 VALU.
// TAIL: the tile holds scalar-tail columns (smask != 0xF); such a wave runs
// the per-column form alone, every other wave the SSE2 form alone.
// The arithmetic is resize_tile_direct's: every output byte is the same.
template <bool TAIL>
__device__ inline void resize_tile_uniform(const DevPlan &p, const FrameBufs &fb, int l, const ResizeWave &a,
                                           const ResizeSched &sc, int b, int ty, int tx, int lane, uint32_t cls,
                                           uint32_t rel0, uint32_t rel1, uint32_t rel2) {
    const LevelArgs g = p.la[l], gs = p.la[l - 1];
    const int twg = a.twg, lr = lane >> a.twg_shift, lg = lane & (twg - 1);
    const int TH = (64 >> a.twg_shift) * kResizeK;
    const int xb = tx * 4 * twg + 4 * lg, yb = ty * TH + mul24u(lr, kResizeK);
    if (xb >= g.w) return;
    const __amdgpu_buffer_rsrc_t ct = wave_rsrc(p.rcols + a.col_off), rt = wave_rsrc(p.rrows + a.ytab_off);
    typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
    typedef uint32_t u32x3 __attribute__((ext_vector_type(3)));
    const int co = mul24u(xb, 12);
    const u32x3 cg0 = __builtin_amdgcn_raw_buffer_load_b96(ct, co, 0, 0);     // c, o, smask
    const u32x4 cg1 = __builtin_amdgcn_raw_buffer_load_b128(ct, co + 16, 0, 0);   // sel
    const u32x4 cg2 = __builtin_amdgcn_raw_buffer_load_b128(ct, co + 32, 0, 0);   // coef
    const uint32_t s01 = __builtin_amdgcn_raw_buffer_load_b32(rt, 8 * yb, 0, 0);   // the group's first row
    // The vertical coefficients stay packed (b0 | b1 << 16, one VGPR a row, unpacked to b << 12 by
    // two SDWA shifts a row): as {b0 << 12, b1 << 12} pairs they cost two VALU a row less but ten
    // VGPRs more (112 against 97), and the kernel's register footprint beside k_fast's waves
    // outweighs its own VALU in the pipelined step.
    uint32_t bq[kResizeK];
#pragma unroll
    for (int j = 0; j < kResizeK; ++j) bq[j] = __builtin_amdgcn_raw_buffer_load_b32(rt, 8 * yb + 4, 8 * j, 0);
    int spitch;
    __amdgpu_buffer_rsrc_t src = wave_rsrc(level_ptr(p, fb, l - 1, b, spitch));
    spitch = __builtin_amdgcn_readfirstlane(spitch);
    if (l == 1) {   // (the caller's image: range as in resize_tile_direct)
        const uint64_t a0 = reinterpret_cast<uint64_t>(level_ptr(p, fb, 0, b, spitch));
        const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)a0), hi = __builtin_amdgcn_readfirstlane((uint32_t)(a0 >> 32));
        src = __builtin_amdgcn_make_buffer_rsrc(reinterpret_cast<void *>(((uint64_t)hi << 32) | lo), (short)0,
                                                ((gs.h - 1) * spitch + gs.w + 3) & ~3, 0x00020000);
    }
    const int c = (int)cg0.x, o = (int)cg0.y;
    const uint32_t sel[4] = {cg1.x, cg1.y, cg1.z, cg1.w}, coef[4] = {cg2.x, cg2.y, cg2.z, cg2.w};
    // source row of output row j, relative to the group's first (scalar)
    auto rel = [&](int j) -> int { return (int)(((j < 4 ? rel0 : j < 8 ? rel1 : rel2) >> (8 * (j & 3))) & 0xFFu); };
    auto reuse = [&](int j) -> bool { return j > 0 && (cls >> j & 1u) != 0; };
    const int sbase = mul24u((int)(s01 & 0xFFFFu), spitch) + c;
    u32x3 d0[kResizeK], d1[kResizeK];
#pragma unroll
    for (int j = 0; j < kResizeK; ++j) {
        const int off = rel(j) * spitch;
        if (!reuse(j)) d0[j] = __builtin_amdgcn_raw_buffer_load_b96(src, sbase, off, 0);
        // Only the tile's last row can read the source level's last row, where
        // the buffer's range has to cut the dword past the image: that one
        // load carries its row in the lane offset, which the range check covers
        // whatever it makes of the scalar offset.
        if (j < kResizeK - 1) d1[j] = __builtin_amdgcn_raw_buffer_load_b96(src, sbase, off + spitch, 0);
        else d1[j] = __builtin_amdgcn_raw_buffer_load_b96(src, sbase + (off + spitch), 0, 0);
    }
    const __amdgpu_buffer_rsrc_t dst = wave_rsrc(fb.pyr + (int64_t)b * p.pyr_bytes + g.pyr_off);
    const int dbase = mul24u(yb, g.pitch) + xb;
    auto hrow = [&](u32x3 d, uint32_t h[4]) {
        const uint32_t w0 = __builtin_amdgcn_alignbyte(d.y, d.x, o), w1 = __builtin_amdgcn_alignbyte(d.z, d.y, o);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint32_t pr = __builtin_amdgcn_perm(w1, w0, sel[k]);
            h[k] = __builtin_amdgcn_udot2(__builtin_bit_cast(u16x2_t, pr), __builtin_bit_cast(u16x2_t, coef[k]), 0u,
                                          false);
        }
    };
    uint32_t hp[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int j = 0; j < kResizeK; ++j) {
        uint32_t h0[4], h1[4];
        if (reuse(j)) {
#pragma unroll
            for (int k = 0; k < 4; ++k) h0[k] = hp[k];
        } else {
            hrow(d0[j], h0);
        }
        hrow(d1[j], h1);
#pragma unroll
        for (int k = 0; k < 4; ++k) hp[k] = h1[k];
        uint32_t packed = 0;
        if (!TAIL) {
            packed = resize_vpass_simd(h0, h1, (bq[j] & 0xFFFFu) << 12, (bq[j] >> 16) << 12);
        } else {
            const uint32_t smask = cg0.z, b0 = bq[j] & 0xFFFFu, b1 = bq[j] >> 16;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const uint32_t v = (smask >> k & 1u)
                                       ? ((mul24u(h0[k] >> 4, b0) >> 16) + (mul24u(h1[k] >> 4, b1) >> 16) + 2) >> 2
                                       : (mul24u(h0[k], b0) + mul24u(h1[k], b1) + (1 << 21)) >> 22;
                packed |= v << (8 * k);
            }
        }
        __builtin_amdgcn_raw_buffer_store_b32(packed, dst, dbase, j * g.pitch, 0);
    }
}

__global__ __launch_bounds__(kThreads) void k_resize_d(DevPlan p, FrameBufs fb, int l, ResizeWave a, int B, ResizeSched sc) {
    const int wave = wave_id(), lane = threadIdx.x & 63;
    const int L = xcd_logical_block(blockIdx.x, gridDim.x);
    const int t = L * 4 + wave;
    if (t >= a.ntiles * B) return;
    const int b = t / a.ntiles, tile = t - b * a.ntiles;
    if (sc.on) {
        // the tile row's class and row schedule: one scalar load from the tile index
        const int ty = tile / a.ntx, tx = tile - ty * a.ntx;
        const uint4 tr = *reinterpret_cast<const uint4 *>(p.rrows + sc.tile_off + 2 * ty);
        uint32_t cls = __builtin_amdgcn_readfirstlane(tr.x), r0 = __builtin_amdgcn_readfirstlane(tr.y),
                 r1 = __builtin_amdgcn_readfirstlane(tr.z), r2 = __builtin_amdgcn_readfirstlane(tr.w);
        // (all four words here: one s_load_dwordx4, not the class first and the rows after a second wait)
        asm volatile("" : "+s"(cls), "+s"(r0), "+s"(r1), "+s"(r2));
        if (cls >> 31) {
            if (tx >= sc.tail_tx) resize_tile_uniform<true>(p, fb, l, a, sc, b, ty, tx, lane, cls, r0, r1, r2);
            else resize_tile_uniform<false>(p, fb, l, a, sc, b, ty, tx, lane, cls, r0, r1, r2);
            return;
        }
    }
    resize_tile_direct(p, fb, l, a, b, tile, lane);
}

// ===========================================================================
// K1 (regions): the whole pyramid of a frame in one launch for small batches.
// Block (region r, frame b) computes levels 1.. of its region with the level
// before each held in LDS: the level-l rectangle R_l it computes is its owned
// rectangle O_l plus what R_{l+1} reads (host plan, plan_pyr_regions), so the
// regions recompute their halos instead of waiting for each other, and only
// O_l is written to the pyramid.  Every pixel is the same fixed-point
// function of the same source pixels as in k_resize (identical output); the
// chain of 7 dependent launches becomes one.
// ===========================================================================
constexpr int kRgnThreads = 1024;
constexpr int kRgnCols = 4;   // computed rectangles are at most 64 * kRgnCols wide (plan_pyr_regions)
constexpr int kRgnTapRows = 64 * kRgnCols;   // and at most this tall
// LDS of the taps of levels 1.. (columns then rows of each)
constexpr int rgn_tap_bytes(int nlevels) { return (int)sizeof(ResizeTap) * 2 * kRgnTapRows * (nlevels - 1); }

// A workgroup barrier that orders LDS only: the kernel's global stores are
// read by later launches, so waiting for them at every level (as
// __syncthreads' release does) would only add their write latency.
__device__ inline void lds_barrier() { __asm__ volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

__global__ __launch_bounds__(kRgnThreads) void k_pyramid_rgn(DevPlan p, FrameBufs fb) {
    extern __shared__ __align__(16) uint8_t lds[];
    const int r = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const int wave = tid >> 6, lane = tid & 63;
    constexpr int kWaves = kRgnThreads / 64;
    const int4 *T = p.pyr_rgn + (int64_t)r * 2 * kMaxLevels;   // [l] = R_l, [kMaxLevels + l] = O_l
    uint8_t *cur = lds, *nxt = lds + p.pyr_rgn_half;
    // every level's taps for this region's columns and rows, staged with R_0 so
    // the level loop issues no global loads (on gfx9 a wait for a load also
    // waits for the level's earlier global stores)
    ResizeTap *sxt = reinterpret_cast<ResizeTap *>(lds + 2 * p.pyr_rgn_half);
    ResizeTap *syt = sxt + kRgnTapRows * (p.nlevels - 1);
    for (int i = tid; i < 2 * kRgnTapRows * (p.nlevels - 1); i += kRgnThreads) {
        const int ly = i >= kRgnTapRows * (p.nlevels - 1);
        const int j = i - ly * kRgnTapRows * (p.nlevels - 1);
        const int l = 1 + j / kRgnTapRows, k = j - (l - 1) * kRgnTapRows;
        const int4 Rl = T[l];
        const LevelGeom &g = p.lv[l];
        if (!ly && k <= Rl.z - Rl.x) sxt[j] = p.xtaps[g.xtab_off + Rl.x + k];
        if (ly && k <= Rl.w - Rl.y) syt[j] = p.ytaps[g.ytab_off + Rl.y + k];
    }
    // R_0 from level 0, dword-aligned rows (level 0's base and pitch are dword multiples)
    int4 R = T[0];
    int ox = R.x & ~3, oy = R.y;
    int stride;
    {
        int sp;
        const uint8_t *src = level_ptr(p, fb, 0, b, sp);
        const int ndw = ((R.z - ox) >> 2) + 1, nrows = R.w - R.y + 1;
        stride = 4 * ndw + 4;
        for (int row = wave; row < nrows; row += kWaves) {
            const uint32_t *s32 = reinterpret_cast<const uint32_t *>(src + (int64_t)(oy + row) * sp + ox);
            uint32_t *d32 = reinterpret_cast<uint32_t *>(cur + row * stride);
            for (int d = lane; d < ndw; d += 64) d32[d] = s32[d];
        }
    }
    lds_barrier();
    for (int l = 1; l < p.nlevels; ++l) {
        const int4 Rl = T[l], Ol = T[kMaxLevels + l];
        const LevelArgs g = p.la[l];
        const int gsh = p.la[l - 1].h;
        const ResizeTap *xt = sxt + kRgnTapRows * (l - 1);
        const ResizeTap *yt = syt + kRgnTapRows * (l - 1);
        const int w = Rl.z - Rl.x + 1, h = Rl.w - Rl.y + 1;
        const int dstride = (w + 4 + 3) & ~3;
        uint8_t *dst = fb.pyr + (int64_t)b * p.pyr_bytes + g.pyr_off;
        // this lane's columns lane + 64 k (k < kRgnCols: the plan bounds the
        // widths) and their taps, read once for all rows
        ResizeTap tx[kRgnCols];
#pragma unroll
        for (int k = 0; k < kRgnCols; ++k) tx[k] = xt[min(lane + 64 * k, w - 1)];
        for (int row = wave; row < h; row += kWaves) {
            const int y = Rl.y + row;
            const ResizeTap ty = yt[row];
            const int s0 = min(max((int)ty.src, 0), gsh - 1) - oy, s1 = min(max((int)ty.src + 1, 0), gsh - 1) - oy;
            const uint8_t *S0 = cur + s0 * stride - ox, *S1 = cur + s1 * stride - ox;
            const int b0 = ty.a0, b1 = ty.a1;
            const bool own_row = y >= Ol.y && y <= Ol.w;
#pragma unroll
            for (int k = 0; k < kRgnCols; ++k) {
                const int col = lane + 64 * k;
                if (col >= w) break;
                const int x = Rl.x + col;
                const int sx = tx[k].src;
                const int h0 = mul24u(S0[sx], tx[k].a0) + mul24u(S0[sx + 1], tx[k].a1);
                const int h1 = mul24u(S1[sx], tx[k].a0) + mul24u(S1[sx + 1], tx[k].a1);
                const int v_simd = ((mul24u(h0 >> 4, b0) >> 16) + (mul24u(h1 >> 4, b1) >> 16) + 2) >> 2;
                const int v_tail = (mul24u(h0, b0) + mul24u(h1, b1) + (1 << 21)) >> 22;
                const uint8_t v = (uint8_t)min(max((tx[k].mode & 2) ? v_simd : v_tail, 0), 255);
                nxt[row * dstride + col] = v;
                if (own_row && x >= Ol.x && x <= Ol.z) dst[(int64_t)y * g.pitch + x] = v;
            }
        }
        lds_barrier();
        uint8_t *t = cur; cur = nxt; nxt = t;
        stride = dstride; ox = Rl.x; oy = Rl.y;
    }
}

}  // namespace

// ---------------------------------------------------------------------------
hipError_t launch_resize_level(const DevPlan &p, const Plan &hp, const FrameBufs &fb, int B, hipStream_t st, int l) {
    if (!hp.rw.empty()) {
        const ResizeWave &a = hp.rw[l];
        const int waves = a.ntiles * B;
        if (a.direct) {
            hipLaunchKernelGGL(k_resize_d, dim3((waves + 3) / 4), dim3(kThreads), 0, st, p, fb, l, a, B, hp.rs[l]);
            return hipGetLastError();
        }
        // one global round trip for the whole window: NB >= the staging's row passes
        if (a.stage_passes <= 9)
            hipLaunchKernelGGL(k_resize_w<9>, dim3((waves + 3) / 4), dim3(kThreads), 4 * a.win_bytes, st, p, fb, l, a, B);
        else if (a.stage_passes <= 16)
            hipLaunchKernelGGL(k_resize_w<16>, dim3((waves + 3) / 4), dim3(kThreads), 4 * a.win_bytes, st, p, fb, l, a, B);
        else
            hipLaunchKernelGGL(k_resize_w<24>, dim3((waves + 3) / 4), dim3(kThreads), 4 * a.win_bytes, st, p, fb, l, a, B);
        return hipGetLastError();
    }
    const LevelGeom &g = hp.lv[l];
    dim3 grid((g.w + kResTW - 1) / kResTW, (g.h + kResTH - 1) / kResTH, B);
    hipLaunchKernelGGL(k_resize, grid, dim3(kThreads), 0, st, p, fb, l);
    return hipGetLastError();
}

hipError_t launch_resize(const DevPlan &p, const Plan &hp, const FrameBufs &fb, int B, hipStream_t st) {
    if (use_pyr_regions(hp, B)) {
        static bool lds_set = false;   // (one attribute per process; the size bound is the plan check's)
        if (!lds_set) {
            if (hipFuncSetAttribute(reinterpret_cast<const void *>(k_pyramid_rgn),
                                    hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) != hipSuccess)
                return hipErrorInvalidValue;
            lds_set = true;
        }
        hipLaunchKernelGGL(k_pyramid_rgn, dim3(hp.rgn_n, B), dim3(kRgnThreads), 2 * hp.rgn_half + rgn_tap_bytes(hp.nlevels), st,
                           p, fb);
        return hipGetLastError();
    }
    for (int l = 1; l < hp.nlevels; ++l)
        if (launch_resize_level(p, hp, fb, B, st, l) != hipSuccess) return hipErrorLaunchFailure;
    return hipSuccess;
}

// Region pyramid plan (k_pyramid_rgn): level 1 cut into ~96 x 96 owned
// rectangles, every level cut at the same fractions; each region's computed
// rectangles grow from the coarsest level down by what the next level reads.
// False (rgn_n = 0) when a region's level buffers exceed the LDS.
bool plan_pyr_regions(Plan &hp) {
    hp.rgn.clear();
    hp.rgn_n = 0;
    hp.rgn_half = 0;
    const int n = hp.nlevels;
    if (n < 2 || n > kMaxLevels) return false;
    const int gx = std::max(1, (hp.lv[1].w + 95) / 96), gy = std::max(1, (hp.lv[1].h + 95) / 96);
    // the source rectangle of level-l output rectangle q (as k_resize reads it)
    auto src_of = [&](int l, const RgnRect &q) {
        const LevelGeom &g = hp.lv[l], &gs = hp.lv[l - 1];
        const ResizeTap *xt = hp.xtaps.data() + g.xtab_off;
        const ResizeTap *yt = hp.ytaps.data() + g.ytab_off;
        RgnRect s{INT_MAX, INT_MAX, -1, -1};
        for (int x = q.x0; x <= q.x1; ++x) {
            s.x0 = std::min(s.x0, (int)xt[x].src);
            s.x1 = std::max(s.x1, std::min((int)xt[x].src + 1, gs.w - 1));
        }
        for (int y = q.y0; y <= q.y1; ++y) {
            s.y0 = std::min(s.y0, std::min(std::max((int)yt[y].src, 0), gs.h - 1));
            s.y1 = std::max(s.y1, std::min(std::max((int)yt[y].src + 1, 0), gs.h - 1));
        }
        return s;
    };
    auto unite = [](const RgnRect &a, const RgnRect &b) {
        return RgnRect{std::min(a.x0, b.x0), std::min(a.y0, b.y0), std::max(a.x1, b.x1), std::max(a.y1, b.y1)};
    };
    std::vector<RgnRect> out((size_t)gx * gy * 2 * kMaxLevels, RgnRect{0, 0, -1, -1});
    size_t half = 0;
    for (int ry = 0; ry < gy; ++ry)
        for (int rx = 0; rx < gx; ++rx) {
            RgnRect *T = out.data() + ((size_t)ry * gx + rx) * 2 * kMaxLevels;
            for (int l = 1; l < n; ++l) {
                const LevelGeom &g = hp.lv[l];
                T[kMaxLevels + l] = RgnRect{(int)((int64_t)rx * g.w / gx), (int)((int64_t)ry * g.h / gy),
                                            (int)((int64_t)(rx + 1) * g.w / gx) - 1,
                                            (int)((int64_t)(ry + 1) * g.h / gy) - 1};
                const RgnRect &o = T[kMaxLevels + l];
                if (o.x1 < o.x0 || o.y1 < o.y0) return false;   // a level narrower than the cut
            }
            T[n - 1] = T[kMaxLevels + n - 1];
            for (int l = n - 2; l >= 1; --l) T[l] = unite(T[kMaxLevels + l], src_of(l + 1, T[l + 1]));
            T[0] = src_of(1, T[1]);
            for (int l = 0; l < n; ++l) {
                const RgnRect &q = T[l];
                if (l > 0 && (q.x1 - q.x0 + 1 > 64 * kRgnCols || q.y1 - q.y0 + 1 > kRgnTapRows)) return false;
                const size_t stride = l == 0 ? 4 * (size_t)(((q.x1 - (q.x0 & ~3)) >> 2) + 1) + 4
                                             : (size_t)((q.x1 - q.x0 + 1 + 4 + 3) & ~3);
                half = std::max(half, stride * (q.y1 - q.y0 + 1));
            }
        }
    half = (half + 15) & ~size_t(15);
    if (2 * half + rgn_tap_bytes(n) > 160 * 1024) return false;
    hp.rgn = std::move(out);
    hp.rgn_n = gx * gy;
    hp.rgn_half = (int)half;
    return true;
}

// The region pyramid while one block per region and frame still leaves the
// chip short of a block per CU.
constexpr int kRgnMax = 256;   // (region blocks a launch may take before the per-level kernels win)
bool use_pyr_regions(const Plan &hp, int B) { return hp.rgn_n > 0 && (int64_t)B * hp.rgn_n <= kRgnMax; }

// Wave-tile geometry of every level (ResizeWave).  False when some level does
// not fit the wave kernel (a column group spanning more than 7 source bytes,
// i.e. scale factors above ~2.3, or a window over the LDS budget); the block
// kernel k_resize then runs instead.
bool plan_resize_waves(Plan &hp) {
    hp.rw.assign(hp.nlevels, ResizeWave{});
    hp.rs.assign(hp.nlevels, ResizeSched{});
    hp.resize_uniform_tiles = hp.resize_fallback_tiles = 0;
    const char *un = std::getenv("ORBX_RESIZE_UNIFORM");   // =0: the per-lane row schedule for every tile
    const bool uniform_on = !(un && un[0] == '0');
    const size_t nrows = hp.ytaps.size();
    for (int l = 1; l < hp.nlevels; ++l) {
        bool direct = hp.lv[l - 1].w >= 8 && !std::getenv("ORBX_RESIZE_LDS");   // =1: windows in LDS
        if (l == 1) {
            hp.rcols.clear();
            // the rows, then the tile rows' records (appended per level)
            hp.rrows.assign(nrows, ResizeRow{});
        }
        const LevelGeom &g = hp.lv[l], &gs = hp.lv[l - 1];
        const ResizeTap *xt = hp.xtaps.data() + g.xtab_off;
        const ResizeTap *yt = hp.ytaps.data() + g.ytab_off;
        ResizeWave a;
        a.xtab_off = g.xtab_off;
        a.ytab_off = g.ytab_off;
        a.sx = 1. / ((double)g.w / gs.w);
        a.sy = 1. / ((double)g.h / gs.h);
        int best = -1;
        for (int sh = 6; sh >= 4; --sh) {
            const int cols = 4 << sh, n = (g.w + cols - 1) / cols;
            if (best < 0 || n * cols < best) { best = n * cols; a.twg_shift = sh; }
        }
        a.twg = 1 << a.twg_shift;
        const int TW = 4 * a.twg, TH = (64 >> a.twg_shift) * kResizeK;
        a.ntx = (g.w + TW - 1) / TW;
        const int nty = (g.h + TH - 1) / TH;
        a.ntiles = a.ntx * nty;
        int nd_max = 0, nd_win = 0;
        int tail_tx = INT_MAX;   // first tile column with a scalar-tail column group
        a.col_off = (int)hp.rcols.size();   // one ResizeCol per 4 columns, x / 4
        for (int tx = 0; tx < a.ntx; ++tx) {
            const int x0 = tx * TW, xl = std::min(x0 + TW, g.w) - 1;
            const int c_lo = std::min(std::max(resize_src_raw(x0, a.sx), 0), gs.w - 1);
            const int c_hi = std::min(std::max(resize_src_raw(xl, a.sx), 0) + 1, gs.w - 1);
            // the kernel's arithmetic bounds must be the tables' (and cover them)
            if (c_lo != xt[x0].src || c_hi < std::min((int)xt[xl].src + 1, gs.w - 1)) return false;
            nd_win = std::max(nd_win, ((c_lo & 3) + c_hi - c_lo + 1 + 3) >> 2);
            nd_max = std::max(nd_max, nd_win);
            for (int xb = x0; xb <= xl; xb += 4) {
                const int s0 = xt[xb].src, s3 = xt[std::min(xb + 3, g.w - 1)].src;
                if (s3 - s0 + 1 > 7) return false;   // pair bytes within the 8 realigned ones
                nd_max = std::max(nd_max, ((s0 - (c_lo & ~3)) >> 2) + 3);
                // k_resize_d: the 8 bytes from cs = min(s0, w_src - 8) hold every
                // pair byte whose coefficient is not 0 (resize_tile_direct)
                const int cs = std::min(s0, gs.w - 8);
                ResizeCol rc{};
                rc.c = cs & ~3;
                rc.o = cs & 3;
                for (int k = 0; k < 4; ++k) {
                    const ResizeTap &t = xt[std::min(xb + k, g.w - 1)];
                    const int r = t.src - cs;
                    if (r < 0 || r > 7 || (r == 7 && t.a1 != 0)) direct = false;
                    rc.sel[k] = (uint32_t)(r & 7) | 0x0C00u | ((uint32_t)(r < 7 ? r + 1 : 0x0C) << 16) | 0x0C000000u;
                    rc.coef[k] = (uint32_t)(uint16_t)t.a0 | ((uint32_t)(uint16_t)t.a1 << 16);
                    rc.smask |= (t.mode & 2) ? 1 << k : 0;
                }
                if (rc.smask != 0xF) tail_tx = std::min(tail_tx, tx);
                hp.rcols.push_back(rc);
            }
        }
        for (int y = 0; y < g.h; ++y) {
            ResizeRow &rr = hp.rrows[g.ytab_off + y];
            rr.s01 = (uint32_t)std::min(std::max((int)yt[y].src, 0), gs.h - 1) |
                     (uint32_t)std::min(std::max((int)yt[y].src + 1, 0), gs.h - 1) << 16;
            rr.b01 = ((uint32_t)yt[y].a0 & 0xFFFu) | ((uint32_t)yt[y].a1 & 0xFFFu) << 16;
        }
        // The tile rows' classes (ResizeTileRow).  Phase-uniform: every lane
        // group's kResizeK rows inside the level, no source row clamped, and
        // one sequence of source-row steps (each >= 1) shared by the groups.
        ResizeSched sc;
        sc.tile_off = (int)hp.rrows.size();
        sc.tail_tx = tail_tx;
        int n_uniform = 0;
        for (int ty = 0; ty < nty; ++ty) {
            const int y0 = ty * TH;
            ResizeTileRow tr{};
            bool uni = uniform_on && direct && y0 + TH <= g.h;
            for (int y = y0; uni && y < y0 + TH; ++y) uni = yt[y].src >= 0 && yt[y].src + 1 <= gs.h - 1;
            for (int lr = 0; uni && lr < TH / kResizeK; ++lr)
                for (int j = 1; j < kResizeK; ++j) {
                    const int r0 = yt[y0 + j].src - yt[y0].src;
                    const int r = yt[y0 + lr * kResizeK + j].src - yt[y0 + lr * kResizeK].src;
                    const int step = yt[y0 + j].src - yt[y0 + j - 1].src;
                    if (r != r0 || step < 1 || r0 > 255) { uni = false; break; }
                    if (lr == 0) {
                        tr.rel[j >> 2] |= (uint32_t)r0 << (8 * (j & 3));
                        tr.cls |= step == 1 ? 1u << j : 0u;
                    }
                }
            if (uni) tr.cls |= 1u << 31; else tr = ResizeTileRow{};
            n_uniform += uni;
            static_assert(sizeof(ResizeTileRow) == 2 * sizeof(ResizeRow), "a tile row's record is two row slots");
            hp.rrows.push_back(ResizeRow{tr.cls, tr.rel[0]});
            hp.rrows.push_back(ResizeRow{tr.rel[1], tr.rel[2]});
        }
        sc.on = n_uniform > 0;
        hp.rs[l] = sc;
        hp.resize_uniform_tiles += n_uniform * a.ntx;
        hp.resize_fallback_tiles += (nty - n_uniform) * a.ntx;
        int nr_max = 0;
        for (int ty = 0; ty < nty; ++ty) {
            const int y0 = ty * TH, yl = std::min(y0 + TH, g.h) - 1;
            const int r_lo = std::min(std::max(resize_src_raw(y0, a.sy), 0), gs.h - 1);
            const int r_hi = std::min(std::max(resize_src_raw(yl, a.sy) + 1, 0), gs.h - 1);
            for (int y = y0; y <= yl; ++y) {
                const int s0 = std::min(std::max((int)yt[y].src, 0), gs.h - 1);
                const int s1 = std::min(std::max((int)yt[y].src + 1, 0), gs.h - 1);
                if (s0 < r_lo || s1 > r_hi) return false;
            }
            nr_max = std::max(nr_max, r_hi - r_lo + 1);
        }
        a.win_stride = 4 * nd_max;
        a.win_dwords = nr_max * nd_win;
        a.stage_passes = nd_win <= 64 ? (nr_max + 64 / nd_win - 1) / (64 / nd_win) : nr_max;
        a.win_bytes = (nr_max * a.win_stride + 15) & ~15;
        if (4 * a.win_bytes > 64 * 1024) return false;
        a.direct = direct;
        hp.rw[l] = a;
    }
    return true;
}

bool resize_window_fits(const Plan &hp) {
    for (int l = 1; l < hp.nlevels; ++l) {
        const LevelGeom &g = hp.lv[l];
        for (int x0 = 0; x0 < g.w; x0 += kResTW) {
            const int xl = std::min(x0 + kResTW, g.w) - 1;
            if (hp.xtaps[g.xtab_off + xl].src + 8 - hp.xtaps[g.xtab_off + x0].src > kResCols) return false;
        }
        for (int y0 = 0; y0 < g.h; y0 += kResTH) {
            const int yl = std::min(y0 + kResTH, g.h) - 1;
            if (hp.ytaps[g.ytab_off + yl].src + 2 - hp.ytaps[g.ytab_off + y0].src > kResRows) return false;
        }
    }
    return true;
}

}  // namespace orbx
