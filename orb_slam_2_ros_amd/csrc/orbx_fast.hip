// orbx_fast.hip -- per-cell FAST-9 of the ORB extractor on gfx950.
//
// Stage                       reference (wjjcdy/orb_slam_2_ros)
//   k_fast     (all cells)    cell loop + cv::FAST, ORBextractor.cc:820-863
#include "orbx_extract_util.h"

namespace orbx {

#ifdef ORBX_PHASE_PROF
// this stage's phase counters (orbx_extract_util.h); slots 0..7 of orbx_debug_phase_cycles
namespace {
__device__ unsigned long long g_phase[8][256];
}  // namespace
hipError_t phase_cycles_fast(unsigned long long *out, bool reset) { return phase_read(&g_phase, out, reset); }
#endif

namespace {

// ===========================================================================
// K3: per-cell FAST-9 with the reference's cell semantics, one wave per cell
// (no workgroup barriers: each wave owns its cell's LDS slice).
// For each interior pixel the arc score S = max over the 16 nine-pixel arcs of
// max(min(v - p), min(p - v)); the pixel is a corner at threshold t iff S > t
// and cv::FAST's cornerScore is S - 1.  S is evaluated only
// for pixels that pass a compass pre-test at the pass's threshold.  NMS is the
// strict 3x3 test inside the cell (outside neighbours count 0, as FAST on the
// cell sub-image sees them).  As the reference, a pass at iniThFAST comes
// first and a pass at minThFAST only for a cell it left empty (27 % of the
// level-0 cells of the bench frames); the count word says which list the cell uses (bit 31 =
// minThFAST, ORBextractor.cc:846-850).
// Output: keypoints in row-major order, packed (x | y<<12 | s<<24).
// ===========================================================================
// max over the 16 arcs of 9 of max(min(p) - v, v - max(p)) for circle bytes p.
// Lane pair (p, 255 - p): the minimum of the second half is 255 - max(p).
// Equal to OpenCV's cornerScore<16> arc order (its even-anchored pairs of
// arcs cover all 16 starts); min / max are exact, so any order agrees.

// The 16 arcs in pairs sharing 8 points (as OpenCV's cornerScore<16> walks
// them): for even k, arcs k..k+8 and k+1..k+9 are the block B = k+1..k+8 plus
// point k or point k+9.  The eight blocks (odd starts j) come from minima of
// pairs and quads at odd starts only: 24 + 24 packed ops (the 16 arcs' minima
// folded per block) instead of the 48 + 16 + 15 of all sixteen sliding windows.
// Block i = points 2i+1 .. 2i+8 (minimum m8) serves the arcs starting at 2i
// and 2i+1, whose minima max together as min(m8, e[2i]) v min(m8, e[2i+9]) =
// min(m8, max(e[2i], e[2i+9])) (min distributes over max).
// The pairs are offset by K = 0x3C00 (both halves normal positive
// f16 numbers, 1.0 .. 1.25, ordered as their bit patterns), so gfx950's packed
// three-input v_pk_minimum3_f16 / v_pk_maximum3_f16 apply: block i's value is
// min3(m4[i], m4[i+2], max(e[2i], e[2i+9])) (no m8 stage) and the eight block
// values fold by max3 -- 8 + 8 + 16 + 4 packed ops against 8 + 8 + 8 + 24.
__device__ inline u16x2 pk_min3_h(u16x2 a, u16x2 b, u16x2 c) {
    uint32_t r;
    asm("v_pk_minimum3_f16 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return as_u16x2(r);
}
__device__ inline u16x2 pk_max3_h(u16x2 a, u16x2 b, u16x2 c) {
    uint32_t r;
    asm("v_pk_maximum3_f16 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return as_u16x2(r);
}
__device__ inline int arc_score_bytes(const int p[16], int v) {
    constexpr uint32_t K = 0x3C00u, C = ((255u + K) << 16) + K;   // (p, 255 - p) + (K, K)
    u16x2 e[16], m2[8], m4[8], x[8];
#pragma unroll
    for (int k = 0; k < 16; ++k) e[k] = as_u16x2(C - (uint32_t)p[k] * 65535u);
#pragma unroll
    for (int i = 0; i < 8; ++i) m2[i] = __builtin_elementwise_min(e[2 * i + 1], e[(2 * i + 2) & 15]);   // j, j+1
#pragma unroll
    for (int i = 0; i < 8; ++i) m4[i] = __builtin_elementwise_min(m2[i], m2[(i + 1) & 7]);              // j..j+3
#pragma unroll
    for (int i = 0; i < 8; ++i)
        x[i] = pk_min3_h(m4[i], m4[(i + 2) & 7], __builtin_elementwise_max(e[2 * i], e[(2 * i + 9) & 15]));
    const u16x2 best = __builtin_elementwise_max(pk_max3_h(pk_max3_h(pk_max3_h(x[0], x[1], x[2]), x[3], x[4]), x[5], x[6]), x[7]);
    return max((int)best.x - (int)K - v, v - (255 + (int)K - (int)best.y));
}

// k_fast's cell + ring: nr rows of nd dwords from column
// x0 - 1, so that column x0 lands at patch column 1 (interior column 0 at
// column 4).  R rows a pass (lanes rl < R, R = 64 / nd from a table: no
// division), 8 passes: every load is issued (the buffer's range ends at the
// rectangle, so rows past nr read zeros -- raw buffers check the lane offset,
// which holds the whole row offset here) and the stores of passes starting at
// or past nr are skipped by uniform branches.  The generic loop's per-load
// and per-store exec masks (~3 scalar instructions and a compare each) go.
// Rows in [nr, nr + R) of the last pass land below the patch, in its spare
// rows or the score map, which each FAST pass zeroes before use; the caller
// checks that 8 R >= nr and that nr + R - 1 rows fit the patch + score map.
__device__ inline int fast_stage_rows(int nd) {   // 64 / nd for nd in [1, 12], 0 past (selects, no division)
    return nd <= 1 ? 64 : nd == 2 ? 32 : nd == 3 ? 21 : nd == 4 ? 16 : nd == 5 ? 12 : nd == 6 ? 10 : nd == 7 ? 9
         : nd == 8 ? 8 : nd == 9 ? 7 : nd == 10 ? 6 : nd <= 12 ? 5 : 0;
}
__device__ inline void stage_fast_patch(uint8_t *dst, int ps, const uint8_t *img, int pitch, int y0, int x0, int nr,
                                        int nd, int R, int lane) {
    const int xs = x0 - 1, xa = xs & ~3, sh = xs - xa;
    const uint64_t a = reinterpret_cast<uint64_t>(img + (int64_t)y0 * pitch + xa);
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)a), hi = __builtin_amdgcn_readfirstlane((uint32_t)(a >> 32));
    const __amdgpu_buffer_rsrc_t src = __builtin_amdgcn_make_buffer_rsrc(
        reinterpret_cast<void *>(((uint64_t)hi << 32) | lo), (short)0, nr * pitch, 0x00020000);
    const int rl = div_small(lane, nd), k = lane - mul24u(rl, nd);
    const int voff = mul24u(rl, pitch) + 4 * k + sh, loff = mul24u(rl, ps) + 4 * k;
    const int Rp = R * pitch, Rs = R * ps;   // (scalar)
    typedef __attribute__((address_space(3))) uint32_t lds_u32;
    if (rl < R) {
        uint32_t v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = __builtin_amdgcn_raw_buffer_load_b32(src, voff + j * Rp, 0, 0);
#pragma unroll
        for (int j = 0; j < 8; ++j) asm volatile("" : "+v"(v[j]));   // (all eight issued before any store)
#pragma unroll
        for (int j = 0; j < 8; ++j)
            if (j * R < nr) *(lds_u32 *)(dst + loff + j * Rs) = v[j];
    }
}

// PIPE: a level's cells in a level-pipelined step (a distinct instantiation so
// profiles tell per-level launches from whole-batch ones).
// PSC: the patch / score-map row stride as a compile-time constant (48 or 64:
// every circle, ring and NMS neighbour offset becomes an LDS immediate), or 0
// for the launch's runtime stride.
template <bool PIPE, int PSC>
__global__ __launch_bounds__(kThreads) void k_fast(DevPlan p, FrameBufs fb, int c0, int nc, FastLds fl,
                                                   uint32_t gmagic) {
    extern __shared__ __align__(16) uint8_t lds[];
    PHASE_START();
    const int wave = wave_id(), lane = threadIdx.x & 63;
    int bx, b;
    xcd_block_2d(bx, b, gmagic);
    if (bx * 4 + wave >= nc) return;
    const int ci = c0 + bx * 4 + wave;
    // the cell as five dwords: scalar loads (a 16-bit field would take a
    // vector load, and a vector round trip, ahead of the staging)
    static_assert(sizeof(Cell) == 20, "five dwords");
    Cell c;
    {
        const uint32_t *cp = reinterpret_cast<const uint32_t *>(p.cells) + 5 * ci;
        const uint32_t w0 = cp[0], w1 = cp[1], w2 = cp[2];
        c.level = (int16_t)(w0 & 0xFFFFu);
        c.pad = 0;
        c.x0 = (int16_t)(w1 & 0xFFFFu);
        c.y0 = (int16_t)(w1 >> 16);
        c.x1 = (int16_t)(w2 & 0xFFFFu);
        c.y1 = (int16_t)(w2 >> 16);
        c.slot = (int32_t)cp[3];
        c.cap = (int32_t)cp[4];
    }
    int32_t *count_out = fb.cell_count + (int64_t)b * p.ncells + ci;
    const int cw = c.x1 - c.x0, ch = c.y1 - c.y0;
    if (cw <= 0 || ch <= 0) {
        if (lane == 0) *count_out = 0;
        return;
    }
    // the patch and the score map share the row stride (fast_lds)
    const int PS = PSC ? PSC : fl.ps;
    const int pmag = PSC ? (int)(((1u << 24) + PSC - 1) / (PSC ? PSC : 1)) : fl.pmag;
    const int kxy0 = c.x0 + (c.y0 << 12);   // pack_key of interior pixel (0, 0), score 0
    uint8_t *patch = lds + (size_t)wave * fl.per_wave;
    uint8_t *scm = patch + fl.patch_bytes;   // S-1 of the pass's corners, 0 elsewhere
    // survivors and corners as patch offsets yy * PS + xx from interior pixel
    // (0, 0) (the score map's index of the pixel is the same + PS + 1), row-major
    uint16_t *list = reinterpret_cast<uint16_t *>(scm + fl.score_bytes);
    int spitch;
    const uint8_t *img = level_ptr(p, fb, c.level, b, spitch);
    // (the cell is staged so that interior column 0 lands on
    // a dword boundary (patch column 4, loads unaligned): a 31-pixel cell row
    // is then 8 quads, 4 lane groups, 16 rows per compass step, where a
    // misaligned one took 9 quads, 5 groups, 12 rows: 2.66 -> 2.06 compass
    // steps per VGA cell)
    int o;
    {
        const int sp = __builtin_amdgcn_readfirstlane(spitch), nr = ch + 6;
        const int nd = (1 + cw + 6 + 3) >> 2;
        const int R = fast_stage_rows(nd);
        if (R && 8 * R >= nr && (nr + R - 1) * PS <= fl.patch_bytes + fl.score_bytes) {
            stage_fast_patch(patch, PS, img, sp, c.y0 - 3, c.x0 - 3, nr, nd, R, lane);
            o = 1;
        } else {
            o = wave_stage_rows<8, true, false, 1>(patch, PS, img, spitch, c.y0 - 3, c.x0 - 3, nr, cw + 6, lane);
        }
    }
    const uint8_t *pc = patch + 3 * PS + o + 3;         // interior pixel (0, 0)
    PHASE_MARK(0, 0);   // prologue + staging
    if constexpr (kStopFast == 1) {
        if (lane == 0) *count_out = 0;
        return;
    }
    uint32_t *out_i = fb.cand + (int64_t)b * p.cand_cap + c.slot;
    uint32_t *out_m = fb.cand2 + (int64_t)b * p.cand_cap + c.slot;
    // The compass pass's lane geometry (both passes): lane = (row in pass,
    // quad of the row), 64 / nq rows per pass; a lane keeps its quad column,
    // so its interior mask is fixed.
    const int qc0 = (o + 3) & ~3;                           // patch column of the first quad
    const int nq = ((o + 2 + cw) >> 2) - (qc0 >> 2) + 1;   // quads per row
    // a lane takes kFQ adjacent quads (4 kFQ pixels) of one row: the loads,
    // the loop and the compaction scan are shared by that many pixels
    constexpr int kFQ = 2, kFP = 4 * kFQ;   // (3: 706 VALU per wave against 698, same time)
    const int np = kFQ == 2 ? (nq + 1) >> 1 : div_small(nq + kFQ - 1, kFQ);   // quad groups per row
    const int R = __builtin_amdgcn_readfirstlane(div_small(64, np));
    const int rl = div_small(lane, np), pi = lane - mul24u(rl, np);
    const int xx0 = qc0 - o - 3 + kFP * pi;   // interior x of the group's byte 0
    // candidate bits: bit j = pixel j of the group; the interior pixels
    // [lo, hi) of the group as one bit field
    const int vlo = min(max(-xx0, 0), kFP), vhi = min(max(cw - xx0, 0), kFP);
    uint32_t vmask = __builtin_amdgcn_ubfe(((1u << kFP) - 1u) << vlo, 0, (uint32_t)vhi);   // bits [lo, hi)
    if (rl >= R) vmask = 0;   // (tail lanes: rows of the next pass)
    // the lane's group in LDS, 3 rows up (every load a non-negative offset
    // from it; 32-bit address arithmetic), and its row limit
    const lds_u8 *qb0 = (const lds_u8 *)(patch + mul24u(rl, PS) + qc0 + kFP * pi);
    const int rlim = mul24u(max(ch - rl, 0), PS);   // (row offsets in bytes: the loop runs on scalars)

    // One FAST pass at threshold th: returns the keypoints kept after NMS,
    // written to out.  The reference runs iniThFAST first and minThFAST only
    // for a cell where that found nothing (ORBextractor.cc:842-850).
    auto pass = [&](int th, uint32_t *out, int ph) -> int {
        {
            uint4 *z0 = reinterpret_cast<uint4 *>(scm);   // (16-B aligned; score_bytes a multiple of 16)
            const int nz = fl.score_bytes >> 4;
            for (int i = lane; i < nz; i += 64) z0[i] = make_uint4(0u, 0u, 0u, 0u);
        }
        wave_lds_fence();
        // The list holds, in row-major order, the corners still waiting for
        // their NMS (list[0, npend): the last scored row's) and then the
        // compass survivors of the rows since (list[npend, npend + nsurv)).
        // It has room for fl.list_cap entries (8 workgroups per CU at VGA,
        // 6 with a list for every pixel of the cell); before a compass step
        // could overflow it, the survivors so far are scored and the corners
        // of every finished row are suppressed and written (flush).
        int npend = 0, nsurv = 0, base = 0;
        // B + C for the survivors in list[npend, npend + nsurv), rows [0, ydone)
        // compass-tested; final: every remaining corner is decided.
        auto flush = [&](int ydone, bool final) {
            // B. arc score of every survivor: S = max(M1 - v, v - M2), M1 = max over
            //    the 16 nine-pixel arcs of the arc's minimum, M2 = min over arcs of the
            //    arc's maximum, side by side as packed u16 lanes (p, 255 - p) through
            //    sliding-window minima (2, 4, 8, 9).  A corner at th iff S > th; its
            //    FAST score S - 1 goes to the map, corners compacted in place.
            // (wave-uniform counts, kept in scalars: loops on scalar compares)
            npend = __builtin_amdgcn_readfirstlane(npend);
            nsurv = __builtin_amdgcn_readfirstlane(nsurv);
            int ncorner = npend;
            for (int i0 = 0; i0 < nsurv; i0 += 64) {
                // every lane scores (no exec region): a lane past the survivors
                // reads a stale entry, or LDS past the list, clamped to entry 0
                // (pixel (0, 0)) so that its circle reads stay inside the patch;
                // it is masked after
                const bool live = i0 + lane < nsurv;
                const int e = live ? (int)list[npend + i0 + lane] : 0;
                const uint8_t *q = pc + e;
                const int v = q[0];
                const uint32_t pr[16] = {q[3 * PS],  q[3 * PS + 1],  q[2 * PS + 2],  q[PS + 3],
                                         q[3],       q[-PS + 3],     q[-2 * PS + 2], q[-3 * PS + 1],
                                         q[-3 * PS], q[-3 * PS - 1], q[-2 * PS - 2], q[-PS - 3],
                                         q[-3],      q[PS - 3],      q[2 * PS - 2],  q[3 * PS - 1]};
                const int S = arc_score_bytes(reinterpret_cast<const int *>(pr), v);
                const bool corner = live & (S > th);
                const uint64_t m = lanes_lt(i0 + lane, nsurv) & lanes_gt(S, th);   // (the ballot of corner)
                if (corner) scm[e + PS + 1] = (uint8_t)(S - 1);
                wave_lds_fence();   // all survivor reads of this chunk precede the in-place writes
                if (corner) list[ncorner + mbcnt64(m)] = (uint16_t)e;
                ncorner += __popcll(m);
            }
            nsurv = 0;
            wave_lds_fence();
            PHASE_MARK(0, ph + 1);   // arc scores
            if constexpr (kStopFast == 3) { npend = 0; return; }
            // C. strict 3x3 NMS inside the cell (outside neighbours and non-corners
            //    score 0), compacted in row-major order; a corner of row ydone - 1
            //    waits for the next rows' scores unless final.
            // (entries are patch offsets ey * PS + ex: row ey is final below ylast * PS)
            const int ylast = final ? INT_MAX : (ydone - 1) * PS;
            int nfin = 0;
            for (int i0 = 0; i0 < ncorner; i0 += 64) {
                // every lane reads (as in B: a lane past the corners clamped to
                // entry 0, inside the score map), masked after
                const bool live = i0 + lane < ncorner;
                const int e = live ? (int)list[i0 + lane] : 0;
                const bool fin = live & (e < ylast);
                const int si = e + PS + 1;
                // the centre and its 8 neighbours read together, compared
                // with their maximum (no short-circuit chain of dependent reads)
                const int sv = scm[si];
                const int n0 = scm[si - 1], n1 = scm[si + 1], n2 = scm[si - PS - 1], n3 = scm[si - PS],
                          n4 = scm[si - PS + 1], n5 = scm[si + PS - 1], n6 = scm[si + PS], n7 = scm[si + PS + 1];
                const int mx = max(max(max(n0, n1), max(n2, n3)), max(max(n4, n5), max(n6, n7)));
                const bool keep = fin & (sv > mx);
                const uint64_t mf = lanes_lt(i0 + lane, ncorner) & lanes_lt(e, ylast);   // (the ballots of fin, keep)
                const uint64_t mk = mf & lanes_gt(sv, mx);
                const int pk = base + mbcnt64(mk);
                // the key from the offset: ey by the 24-bit reciprocal, then
                // x | y << 12 = x0 + (y0 << 12) + e + ey (4096 - PS)
                const int ey = (int)(__umul24((uint32_t)e, (uint32_t)pmag) >> 24);
                if (keep && pk < c.cap) out[pk] = (uint32_t)(kxy0 + e + mul24u(ey, 4096 - PS)) | ((uint32_t)sv << 24);
                base += __popcll(mk);
                nfin += __popcll(mf);
            }
            // the waiting corners (one row: < 64) to the front
            npend = ncorner - nfin;
            if (npend) {
                const int e = lane < npend ? list[nfin + lane] : 0;
                wave_lds_fence();
                if (lane < npend) list[lane] = (uint16_t)e;
                wave_lds_fence();
            }
            PHASE_MARK(0, ph + 2);   // NMS + output
        };
        // A. compass pre-test: an arc of 9 covers two cyclically adjacent points
        //    of {0, 4, 8, 12}, so a pixel is a corner candidate only if some
        //    adjacent pair is all brighter (min of the pair > v + th) or all
        //    darker (max of the pair < v - th).  A lane tests a dword-aligned
        //    quad of 4 pixels from 5 aligned LDS dwords (the +-3 column
        //    neighbours by byte alignment), as two packed u16 pairs (even and
        //    odd pixels); survivors are compacted in row-major order.
        {
            const u16x2 thv = {(unsigned short)th, (unsigned short)th};
            const u16x2 thv8 = {(unsigned short)(th << 8), (unsigned short)(th << 8)};
            typedef __attribute__((address_space(3))) const uint32_t lds_u32c;
            const int e = mul24u(rl, PS) + xx0;   // the list entry of the group's byte 0 at yo = 0
            const int RPS = __builtin_amdgcn_readfirstlane(R * PS);
            const int chps = __builtin_amdgcn_readfirstlane(ch * PS);
            for (int yo = 0, ys = 0; yo < chps; yo += RPS, ys += R) {
                // survivors this step can add: its rows' pixels (wave-uniform)
                if (npend + nsurv + min(R, ch - ys) * cw > fl.list_cap) {
                    if constexpr (kStopFast == 2) nsurv = 0;
                    else flush(ys, false);
                }
                uint32_t cand = 0;
                if (yo < rlim) {
                    const lds_u8 *qb = qb0 + yo;
                    // the group's dwords c[0..kFQ), their row neighbours c[-1] and
                    // c[kFQ], and the rows 3 up / down
                    uint32_t c[kFQ + 2], up[kFQ], dn[kFQ];
#pragma unroll
                    for (int k = 0; k < kFQ + 2; ++k) c[k] = *reinterpret_cast<lds_u32c *>(qb + 3 * PS - 4 + 4 * k);
#pragma unroll
                    for (int k = 0; k < kFQ; ++k) {
                        up[k] = *reinterpret_cast<lds_u32c *>(qb + 4 * k);
                        dn[k] = *reinterpret_cast<lds_u32c *>(qb + 6 * PS + 4 * k);
                    }
                    // one quad: pixel pairs (0, 2) and (1, 3) as u16 halves, straight
                    // from the aligned dwords (v_perm picks the +-3 column bytes of
                    // (lo, hi) dword pairs); even pixels: bytes 0 / 2 as the low bytes
                    // of the halves (an AND for the aligned dwords); odd pixels: bytes
                    // 1 / 3 left in the high bytes, every value and the threshold
                    // scaled by 256 -- the same comparisons, without the shift
                    auto quad = [&](uint32_t c, uint32_t lft, uint32_t rgt, uint32_t up, uint32_t dn) -> uint32_t {
                        // ODD: the pixels sit in the high bytes of the halves and the low
                        // bytes are left as they come (another pixel).  Max / min then
                        // give the right high byte and some low byte h or l, and with the
                        // centre as V:FF against hi and V:00 against lo,
                        //   sat(H:h - V:FF) > th:00  <=>  H - V > th,  sat(V:00 - L:l) > th:00  <=>  V - L > th
                        // (the low-byte terms lie in [-255, 0]): one operand op fewer a half.
                        auto half = [&](auto odd, uint32_t sel4, uint32_t sel12, u16x2 thv) -> u16x2 {   // 1: candidate
                            constexpr bool kOdd = decltype(odd)::value;
                            const u16x2 vh = as_u16x2(kOdd ? (c | 0x00FF00FFu) : (c & 0x00FF00FFu));   // (v against hi)
                            const u16x2 vl = kOdd ? as_u16x2(c & 0xFF00FF00u) : vh;                  // (v against lo)
                            const u16x2 a0 = as_u16x2(kOdd ? dn : (dn & 0x00FF00FFu));
                            const u16x2 a4 = as_u16x2(__builtin_amdgcn_perm(rgt, c, sel4));    // x + 3
                            const u16x2 a8 = as_u16x2(kOdd ? up : (up & 0x00FF00FFu));
                            const u16x2 a12 = as_u16x2(__builtin_amdgcn_perm(c, lft, sel12));  // x - 3
                            // max over the cyclic pairs of the pair's min, and min of the max:
                            // max(min(a,b), min(b,c), min(c,d), min(d,a)) = min(max(a,c), max(b,d))
                            const u16x2 hi = __builtin_elementwise_min(__builtin_elementwise_max(a0, a8),
                                                                       __builtin_elementwise_max(a4, a12));
                            const u16x2 lo = __builtin_elementwise_max(__builtin_elementwise_min(a0, a8),
                                                                       __builtin_elementwise_min(a4, a12));
                            // hi > v + th  or  lo + th < v  <=>  max(hi - v, v - lo) > th (saturating)
                            const u16x2 d = __builtin_elementwise_sub_sat(
                                __builtin_elementwise_max(__builtin_elementwise_sub_sat(hi, vh),
                                                          __builtin_elementwise_sub_sat(vl, lo)),
                                thv);
                            u16x2 m;   // min(d, 1) per half, kept one packed op
                            asm("v_pk_min_u16 %0, %1, %2" : "=v"(m) : "v"(d), "s"(0x00010001u));
                            return m;
                        };
                        // pixels 0 / 2 at bits 0 / 16, 1 / 3 at bits 1 / 17
                        return __builtin_bit_cast(uint32_t, half(std::false_type{}, 0x0c050c03u, 0x0c030c01u, thv)) |
                               (__builtin_bit_cast(uint32_t, half(std::true_type{}, 0x060c040cu, 0x040c020cu, thv8)) << 1);
                    };
                    // quad k's pixels 0 / 2 at bits 4k / 4k + 16, 1 / 3 at 4k + 1 / 4k + 17,
                    // folded to bits 4k .. 4k + 3
                    uint32_t bits = 0;
#pragma unroll
                    for (int k = 0; k < kFQ; ++k) bits |= quad(c[k + 1], c[k], c[k + 2], up[k], dn[k]) << (4 * k);
                    cand = (bits | (bits >> 14)) & vmask;
                }
                // compaction in row-major order: an inclusive DPP scan of the
                // lanes' counts (0..4 kFQ) places each lane's run, then its bits
                const int cnt = __builtin_popcount(cand);
                const int incl = wave_incl_scan_i32_to(cnt);
                const int total = __builtin_amdgcn_readlane(incl, 63);
                if (total) {
                    typedef __attribute__((address_space(3))) uint16_t lds_u16;
                    lds_u16 *dst = (lds_u16 *)list + npend + nsurv + (incl - cnt);
                    const int ey = e + yo;
                    // the lane's k-th bit to dst[k] (LDS immediate offsets), while any lane has one
#pragma unroll
                    for (int k = 0; k < kFP; ++k) {
                        if (!__builtin_amdgcn_ballot_w64(cand != 0u)) break;
                        if (cand) {
                            dst[k] = (uint16_t)(ey + __builtin_ctz(cand));
                            cand &= cand - 1u;
                        }
                    }
                    nsurv += total;
                }
            }
        }
        wave_lds_fence();
        PHASE_MARK(0, ph);       // score-map zeroing + compass pre-test + compaction
        if constexpr (kStopFast == 2) return 0;
        flush(ch, true);
        return base;
    };
    const int n_ini = pass(p.ini_th, out_i, 1);
    int32_t cnt;
    if (n_ini > 0 || (kStopFast >= 2 && kStopFast <= 4)) {
        cnt = min(n_ini, c.cap);
    } else {
        wave_lds_fence();
        const int n_min = pass(p.min_th, out_m, 4);
        cnt = (int32_t)(0x80000000u | (uint32_t)min(n_min, c.cap));
    }
    if (lane == 0) *count_out = cnt;
}

}  // namespace

constexpr int kFastListCap = 640;   // (survivor-list entries, at least what a compass step needs)
FastLds fast_lds(int mw, int mh) {
    FastLds f;
    // survivor-list capacity: every pixel of the largest cell, or 640.  It
    // must hold a row of waiting corners plus what one compass step can add,
    // R rows of cw pixels (k_fast flushes before a step could overflow it):
    // R = 64 / the lane groups of a row, (quads + 1) / 2 for the aligned
    // staging's (cw + 3) / 4 quads (the unaligned fallback has more groups,
    // fewer rows); 527 at VGA.  (Sized to that, 528, the launch fits 9
    // workgroups per CU instead of 8 and measured slower: 2.61 -> 2.70 ms;
    // 7 and 6 workgroups 2.71 and 2.88, profiles/r05_ab_fast_occupancy.txt.)
    int need = 0;
    for (int cw = 1; cw <= mw; ++cw) {
        const int nq = (cw + 3) >> 2, np = (nq + 1) >> 1, R = 64 / np;
        need = std::max(need, (R + 1) * cw);
    }
    f.list_cap = std::min(mw * mh, std::max(kFastListCap, (need + 7) & ~7));
    f.ps = (mw + 6 + 3 + 3) & ~3;   // + alignment offset, dword rows
    // the compass's last lane group reads up to column 4 + 8 ceil(mw / 8) + 3
    // (interior column 0 at patch column 4)
    f.ps = std::max(f.ps, 8 * ((mw + 7) / 8) + 8);
    if (f.ps <= 64) f.ps = f.ps <= 48 ? 48 : 64;   // k_fast's constant-stride instantiations
    // the score map at the patch's stride: a survivor's list entry, its patch
    // offset ey * ps + ex from interior pixel (0, 0), also indexes the map
    // (cells are under 60 px a side, ORBextractor.cc:796-817: offsets < 2^13)
    f.sw = f.ps;
    f.pmag = (int)(((1u << 24) + f.ps - 1) / f.ps);
    f.patch_bytes = (f.ps * (mh + 6) + 15) & ~15;
    f.score_bytes = (f.sw * (mh + 2) + 15) & ~15;
    f.per_wave = f.patch_bytes + f.score_bytes + ((2 * f.list_cap + 15) & ~15);
    return f;
}

namespace {
// The levels [l0, l1)'s cells with LDS sized by their largest cell.
template <bool PIPE>
hipError_t launch_fast_range(const DevPlan &p, const Plan &hp, const FrameBufs &fb, int B, hipStream_t st, int l0,
                             int l1) {
    const int c0 = hp.lv[l0].cell_begin, nc = hp.lv[l1 - 1].cell_end - c0;
    if (nc <= 0) return hipSuccess;
    int mw = 1, mh = 1;
    for (int c = c0; c < c0 + nc; ++c) {
        mw = std::max(mw, hp.cells[c].x1 - hp.cells[c].x0);
        mh = std::max(mh, hp.cells[c].y1 - hp.cells[c].y0);
    }
    const FastLds fl = fast_lds(mw, mh);
    const dim3 grid((nc + 3) / 4, B);
    const uint32_t gm = grid_magic(grid.x, grid.y);
    if (fl.ps == 48 && fl.sw == 48)
        hipLaunchKernelGGL((k_fast<PIPE, 48>), grid, dim3(kThreads), 4 * fl.per_wave, st, p, fb, c0, nc, fl, gm);
    else if (fl.ps == 64 && fl.sw == 64)
        hipLaunchKernelGGL((k_fast<PIPE, 64>), grid, dim3(kThreads), 4 * fl.per_wave, st, p, fb, c0, nc, fl, gm);
    else
        hipLaunchKernelGGL((k_fast<PIPE, 0>), grid, dim3(kThreads), 4 * fl.per_wave, st, p, fb, c0, nc, fl, gm);
    return hipGetLastError();
}

}  // namespace

// All cells of all levels in one launch (one dispatch per stage keeps the
// per-launch roofline figure clean; splitting by cell size measured +1 %).
hipError_t launch_fast(const DevPlan &p, const Plan &hp, const FrameBufs &fb, int B, hipStream_t st) {
    return launch_fast_range<false>(p, hp, fb, B, st, 0, hp.nlevels);
}

hipError_t launch_fast_level(const DevPlan &p, const Plan &hp, const FrameBufs &fb, int B, hipStream_t st, int l,
                             int l_end) {
    return launch_fast_range<true>(p, hp, fb, B, st, l, l_end);
}

#ifdef ORBX_PHASE_PROF
// out[8 k + i] = phase i of kernel k (0 fast, 1 describe, 2 quadtree), in cycles summed over the waves.
extern "C" int orbx_debug_phase_cycles(unsigned long long *out, int cap, int reset) {
    unsigned long long t[24];
    if (phase_cycles_fast(t, reset != 0) != hipSuccess || phase_cycles_describe(t + 8, reset != 0) != hipSuccess ||
        phase_cycles_quadtree(t + 16, reset != 0) != hipSuccess)
        return -5;
    for (int i = 0; i < 24 && i < cap; ++i) out[i] = t[i];
    return 24;
}
#endif

}  // namespace orbx
