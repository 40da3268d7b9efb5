// orbx_quadtree.hip -- keypoint distribution of the ORB extractor on gfx950.
//
// Stage                       reference (wjjcdy/orb_slam_2_ros)
//   k_quadtree (frame,level)  DistributeOctTree, ORBextractor.cc:561-787
#include "orbx_extract_util.h"

namespace orbx {

#ifdef ORBX_PHASE_PROF
// this stage's phase counters (orbx_extract_util.h); slots 16..23 of orbx_debug_phase_cycles
namespace {
__device__ unsigned long long g_phase[8][256];
}  // namespace
hipError_t phase_cycles_quadtree(unsigned long long *out, bool reset) { return phase_read(&g_phase, out, reset); }
#endif

namespace {

// ===========================================================================
// K4: DistributeOctTree, one 256-thread workgroup per (level, frame).
// The reference's std::list is replaced by node arrays rebuilt each round in
// the exact order push_front/erase would leave them:
//   full round:  new list = reverse(children in parent order, n1..n4)
//                           ++ unsplit (single-key) nodes in list order
//   final phase: split the (size, creation) largest first; new list =
//                reverse(children in split order) ++ unsplit nodes in order.
// Keys stay in global scratch (L2-resident); each key carries its node index.
// Size ties in the final phase: later-created node first.
// ===========================================================================
struct QNode {
    int16_t x0, y0, x1, y1;
    int32_t count;
    uint32_t best;   // (score << 24) | (0xFFFFFF - key index): max = best response, first on ties
    int32_t seq;     // creation order among this round's children
};

__device__ inline QNode child_of(const QNode &n, int q) {
    const int hx = (n.x1 - n.x0 + 1) >> 1, hy = (n.y1 - n.y0 + 1) >> 1;
    const int mx = n.x0 + hx, my = n.y0 + hy;
    QNode c;
    c.x0 = (int16_t)((q & 1) ? mx : n.x0);
    c.x1 = (int16_t)((q & 1) ? n.x1 : mx);
    c.y0 = (int16_t)((q & 2) ? my : n.y0);
    c.y1 = (int16_t)((q & 2) ? n.y1 : my);
    c.count = 0;
    c.best = 0;
    c.seq = 0;
    return c;
}

__device__ inline int quadrant_of(const QNode &n, uint32_t key) {
    const int hx = (n.x1 - n.x0 + 1) >> 1, hy = (n.y1 - n.y0 + 1) >> 1;
    const int rx = (int)(key & 0xFFF) - kBorder, ry = (int)((key >> 12) & 0xFFF) - kBorder;
    return (rx < n.x0 + hx ? 0 : 1) | (ry < n.y0 + hy ? 0 : 2);
}

__device__ inline uint32_t best_pack(uint32_t key, int k) {
    return ((key >> 24) << 24) | (uint32_t)(0xFFFFFF - k);
}

struct QLds {
    QNode *cur, *nxt;
    uint32_t *ccnt, *cbest;
    int16_t *nidx_c, *nidx_s;
    uint8_t *mark;
    uint64_t *a64, *b64;
    int np2;
};

// The level's keys, each with its node index and quadrant.  R > 0: thread t
// holds keys t + 256 j (j < R) in registers for the whole distribution (the
// rounds then touch no global memory); R == 0: they stay in global scratch.
// 6 keys per thread cover the bench levels (VGA level 0: ~1300 keys) in 72
// VGPRs (7 waves per SIMD); levels up to kQuadRegKeys take 8 (with spills)
// Per workgroup size NT: register keys per thread on the narrow (R1) and wide
// (R2) paths, the key -> source map's capacity (KR) and workgroups per CU.
// NT = 1024 serves launches too small to fill the chip (a few frames: the
// drop-in call, a sharded camera set), where a level's latency is the step's.
template <int NT> struct QCfg;
// (the register paths counting the roots in the gather too measured slower:
// FHD 0.162 -> 0.164, EuRoC 0.069 -> 0.080 ms, profiles/r04_ab_qt_regroots.txt)
constexpr int kQPreRoots = 16;   // roots the global-key gather counts itself (more: the roots' own pass)
template <> struct QCfg<256> { static constexpr int R1 = 6, R2 = kQuadRegKeys / 256, KR = kQuadRegKeys, MINB = 7; };
template <> struct QCfg<512> { static constexpr int R1 = 10, R2 = 2 * kQuadRegKeysW / 1024, KR = kQuadRegKeysW, MINB = 4; };
template <> struct QCfg<1024> { static constexpr int R1 = 4, R2 = kQuadRegKeysW / 1024, KR = kQuadRegKeysW, MINB = 1; };
// R == 0 (keys in global scratch): a pass walks the keys kQU per thread at a
// time, the chunk's loads issued together into a register cache (key k =
// k0 + u NT + tid: every pass maps a key to the same thread, so its node
// and quadrant need no cross-thread ordering), then the chunk's node and
// quadrant written back.  A key pass is then ~n / (kQU NT) L2 round
// trips instead of n / NT (FHD level 0: ~9.6 k keys, 5 instead of 38).
constexpr int kQU = 4;
template <int R, int NT>
struct QKeys {
    static constexpr int C = R > 0 ? R : kQU;   // registers: the keys, or the chunk cache
    uint32_t key[C];
    uint32_t nq[C];   // node | quadrant << 16
    uint32_t *gkeys;
    uint16_t *gnode;
    uint8_t *gq;
    int n;
    // the chunk at k0 into the cache (R == 0)
    __device__ inline void load(int k0) {
#pragma unroll
        for (int u = 0; u < C; ++u) {
            const int k = k0 + u * NT + (int)threadIdx.x;
            if (k < n) {
                key[u] = gkeys[k];
                // (a key's quadrant is 0..3; masked, as the scratch starts
                // unwritten and an unsplit node's keys read any of its 4 slots)
                nq[u] = (uint32_t)gnode[k] | ((uint32_t)(gq[k] & 3) << 16);
            }
        }
    }
    // body(k0) over every chunk (prefetching the next chunk while the body
    // runs measured slower: FHD quadtree 0.243 -> 0.255 ms, profiles/r04_ab_qt_fhd.txt)
    template <typename B>
    __device__ inline void chunks(B body) {
        for (int k0 = 0; k0 < n; k0 += NT * kQU) {
            load(k0);
            body(k0);
            store(k0);
        }
    }
    __device__ inline void store(int k0) {
#pragma unroll
        for (int u = 0; u < C; ++u) {
            const int k = k0 + u * NT + (int)threadIdx.x;
            if (k < n) {
                gnode[k] = (uint16_t)(nq[u] & 0xFFFF);
                gq[k] = (uint8_t)(nq[u] >> 16);
            }
        }
    }
    // f(j, k) for every key this thread owns
    template <typename F>
    __device__ inline void each(F f) {
        if constexpr (R > 0) {
#pragma unroll
            for (int j = 0; j < R; ++j) {
                const int k = (int)threadIdx.x + j * NT;
                if (k < n) f(j, k);
            }
        } else {
            chunks([&](int k0) {
#pragma unroll
                for (int u = 0; u < kQU; ++u) {
                    const int k = k0 + u * NT + (int)threadIdx.x;
                    if (k < n) f(u, k);
                }
            });
        }
    }
    // f(j, k, valid) on every lane for every key slot (bodies with DPP)
    template <typename F>
    __device__ inline void each_all(F f) {
        if constexpr (R > 0) {
#pragma unroll
            for (int j = 0; j < R; ++j) {
                const int k = (int)threadIdx.x + j * NT;
                f(j, k, k < n);
            }
        } else {
            chunks([&](int k0) {
#pragma unroll
                for (int u = 0; u < kQU; ++u) {
                    const int k = k0 + u * NT + (int)threadIdx.x;
                    f(u, k, k < n);
                }
            });
        }
    }
    __device__ inline uint32_t get_key(int j, int) const { return key[j]; }
    __device__ inline int node(int j, int) const { return (int)(nq[j] & 0xFFFF); }
    __device__ inline int quad(int j, int) const { return (int)(nq[j] >> 16); }
    __device__ inline void set_node(int j, int, int nd) { nq[j] = (nq[j] & 0xFFFF0000u) | (uint32_t)nd; }
    __device__ inline void set_quad(int j, int, int q) { nq[j] = (nq[j] & 0xFFFFu) | ((uint32_t)q << 16); }
};

// Adds each lane's (slot, bp) to cnt[slot] += 1, best[slot] = max(., bp)
// (slot ~0u: nothing) with LDS atomics pre-aggregated over neighbouring
// lanes.  The quadtree's keys sit in cell order, so neighbouring lanes mostly
// hit one slot, and same-address atomics within an instruction serialise in
// the LDS (636 address-conflict cycles per wave before this, 247 after; the
// kernel 0.61 -> 0.38 ms per 3072 VGA frames).  A lane row (16 lanes) or
// quad whose lanes all carry one slot adds its count and maximum from its
// first lane.  Every lane of the wave must call it (DPP).
__device__ inline void agg_atomics(uint32_t *cnt, uint32_t *best, uint32_t slot, uint32_t bp) {
    constexpr int kQX1 = 0xB1, kQX2 = 0x4E;   // quad_perm [1,0,3,2], [2,3,0,1]
    uint32_t lo = min(slot, dpp_or<kQX1>(0u, slot)), hi = max(slot, dpp_or<kQX1>(0u, slot));
    lo = min(lo, dpp_or<kQX2>(0u, lo));
    hi = max(hi, dpp_or<kQX2>(0u, hi));
    uint32_t b4 = max(bp, dpp_or<kQX1>(0u, bp));
    b4 = max(b4, dpp_or<kQX2>(0u, b4));
    const bool quad = lo == hi && slot != ~0u;   // (a mixed quad has lo < hi)
    const int lane = (int)threadIdx.x & 63;
    constexpr int kRor4 = 0x124, kRor8 = 0x128;   // row_ror:4, row_ror:8
    uint32_t rlo = min(lo, dpp_or<kRor4>(0u, lo)), rhi = max(hi, dpp_or<kRor4>(0u, hi));
    rlo = min(rlo, dpp_or<kRor8>(0u, rlo));
    rhi = max(rhi, dpp_or<kRor8>(0u, rhi));
    uint32_t b16 = max(b4, dpp_or<kRor4>(0u, b4));
    b16 = max(b16, dpp_or<kRor8>(0u, b16));
    if (rlo == rhi && slot != ~0u) {
        if ((lane & 15) == 0) {
            atomicAdd(&cnt[slot], 16u);
            atomicMax(&best[slot], b16);
        }
        return;
    }
    if (quad) {
        if ((lane & 3) == 0) {
            atomicAdd(&cnt[slot], 4u);
            atomicMax(&best[slot], b4);
        }
    } else if (slot != ~0u) {
        atomicAdd(&cnt[slot], 1u);
        atomicMax(&best[slot], bp);
    }
}

// Child counts / best keys of the splittable nodes.  ccnt / cbest[0, 4S)
// were zeroed by the step that produced the current nodes (zero_children),
// ordered by that step's closing barrier.  Ends with a barrier.
template <int R, int NT>
__device__ __attribute__((always_inline)) void child_stats(const QLds &s, QKeys<R, NT> &K) {
    // every lane runs each slot's aggregation (lanes past the key count carry
    // slot ~0u)
    K.each_all([&](int j, int k, bool valid) {
        uint32_t slot = ~0u, bp = 0;
        if (valid) {
            const int nd = K.node(j, k);
            const QNode node = s.cur[nd];
            if (node.count > 1) {
                const uint32_t key = K.get_key(j, k);
                const int q = quadrant_of(node, key);
                K.set_quad(j, k, q);
                slot = 4u * (uint32_t)nd + (uint32_t)q;
                bp = best_pack(key, k);
            }
        }
        agg_atomics(s.ccnt, s.cbest, slot, bp);
    });
    __syncthreads();
}

template <int NT>
__device__ inline void zero_children(const QLds &s, int S) {
    for (int i = threadIdx.x; i < 4 * S; i += NT) { s.ccnt[i] = 0; s.cbest[i] = 0; }
}

// One key pass per round: each key moves to its node of the round just built
// (nidx_c[4 node + quadrant]) and, when that node is splittable, adds itself
// to the node's child counts (as child_stats).  Ends with a barrier.  The
// 256-thread form with register-held keys (VGA) moves the keys in a pass of
// their own and then counts (0.386 vs 0.403 ms fused per 3072 VGA frames,
// profiles/r04_ab_qt_fhd2.txt): the fused pass's dependent LDS reads queue
// behind each key's atomics; the global-key path and the wider forms gain from
// the single pass (FHD 0.298 -> 0.243 ms).  (No barrier between the two
// loops: the move touches registers only, and the counters were zeroed before
// the barrier that precedes this pass.)
template <int R, int NT>
__device__ __attribute__((always_inline)) void advance_stats(const QLds &s, QKeys<R, NT> &K) {
    if constexpr (NT == 256 && R > 0) {
        K.each([&](int j, int k) { K.set_node(j, k, s.nidx_c[4 * K.node(j, k) + K.quad(j, k)]); });
        child_stats(s, K);
        return;
    }
    K.each_all([&](int j, int k, bool valid) {
        uint32_t slot = ~0u, bp = 0;
        if (valid) {
            const int nd = s.nidx_c[4 * K.node(j, k) + K.quad(j, k)];
            K.set_node(j, k, nd);
            const QNode node = s.cur[nd];
            if (node.count > 1) {
                const uint32_t key = K.get_key(j, k);
                const int q = quadrant_of(node, key);
                K.set_quad(j, k, q);
                slot = 4u * (uint32_t)nd + (uint32_t)q;
                bp = best_pack(key, k);
            }
        }
        agg_atomics(s.ccnt, s.cbest, slot, bp);
    });
    __syncthreads();
}

// A node that keeps its keys maps all four quadrant slots to its new index,
// so a key's next node is one read, nidx_c[4 node + quadrant], split or not
// (an unsplit node's keys carry a stale quadrant; every slot agrees).
__device__ inline void set_all_quads(int16_t *nidx_c, int i, int ni) {
    const uint32_t v = ((uint32_t)ni & 0xFFFFu) * 0x10001u;
    *reinterpret_cast<uint2 *>(nidx_c + 4 * i) = make_uint2(v, v);
}

__device__ inline QNode make_child(const QLds &s, const QNode &parent, int i, int q, int seq) {
    QNode c = child_of(parent, q);
    c.count = (int32_t)s.ccnt[4 * i + q];
    c.best = s.cbest[4 * i + q];
    c.seq = seq;
    return c;
}

// Phases 2-5 of k_quadtree on the gathered keys (ORBextractor.cc:566-784).
template <int NR, int NT>
__device__ __attribute__((always_inline)) void quadtree_rounds(const DevPlan &p, const FrameBufs &fb, QLds &s, const LevelGeom &g, int b, int l,
                                QKeys<NR, NT> &K, uint64_t &phase_t_, const uint32_t *pre_cnt = nullptr,
                                const uint32_t *pre_best = nullptr) {
    const int tid = threadIdx.x;
    const int N = g.quota, NC = p.node_cap;
    const uint32_t *keys = K.gkeys;
    int32_t *level_count = fb.level_count + (int64_t)b * kMaxLevels + l;
    __shared__ uint64_t ws64[NT / 64];
    __shared__ int sh_S, sh_R, sh_nv;

    // ---- 2. root nodes (ORBextractor.cc:566-613)
    const int nini = g.nini;
    if (pre_cnt) {
        // counted in the gather (every key's node is its root index r, its
        // quadrant 0): the non-empty roots in order, and root r's four slots
        // of nidx_c map to its list position, so the first key pass moves the
        // keys as any round's does (advance_stats)
        for (int i = tid; i < 4 * nini; i += NT) { s.ccnt[i] = 0; s.cbest[i] = 0; }
        if (tid == 0) {
            int S = 0;
            for (int r = 0; r < nini; ++r) {
                if (pre_cnt[r] == 0) continue;
                QNode nd;
                nd.x0 = (int16_t)(int)__fmul_rn(g.hx, (float)r);
                nd.x1 = (int16_t)(int)__fmul_rn(g.hx, (float)(r + 1));
                nd.y0 = 0;
                nd.y1 = (int16_t)(g.h - 2 * kBorder);
                nd.count = (int32_t)pre_cnt[r];
                nd.best = pre_best[r];
                nd.seq = 0;
                s.cur[S] = nd;
                set_all_quads(s.nidx_c, r, S);
                ++S;
            }
            sh_S = S;
        }
        __syncthreads();
    } else if (nini == 1) {
        // one root (every 4:3 or squarer level): every key's node is 0, its
        // count the key count and its best key a block maximum (wave maxima
        // through LDS: no per-key atomics, no serial pass)
        __shared__ uint32_t ws_root[NT / 64];
        uint32_t bm = 0;
        K.each([&](int j, int k) {
            K.set_node(j, k, 0);
            bm = max(bm, best_pack(K.get_key(j, k), k));
        });
        bm = wave_max_u32(bm);
        if ((tid & 63) == 0) ws_root[tid >> 6] = bm;
        zero_children<NT>(s, 1);
        __syncthreads();
        if (tid == 0) {
            QNode nd;
            nd.x0 = (int16_t)(int)__fmul_rn(g.hx, 0.0f);
            nd.x1 = (int16_t)(int)__fmul_rn(g.hx, 1.0f);
            nd.y0 = 0;
            nd.y1 = (int16_t)(g.h - 2 * kBorder);
            nd.count = (int32_t)K.n;
            uint32_t best = 0;
            for (int w = 0; w < NT / 64; ++w) best = max(best, ws_root[w]);
            nd.best = best;
            nd.seq = 0;
            s.cur[0] = nd;
            sh_S = 1;
        }
        __syncthreads();
    } else {
        for (int i = tid; i < nini; i += NT) { s.ccnt[i] = 0; s.cbest[i] = 0; }
        __syncthreads();
        auto root_of = [&](uint32_t key) {
            const float rx = (float)((int)(key & 0xFFF) - kBorder);
            return min((int)__fdiv_rn(rx, g.hx), nini - 1);
        };
        K.each_all([&](int j, int k, bool valid) {
            uint32_t slot = ~0u, bp = 0;
            if (valid) {
                const uint32_t key = K.get_key(j, k);
                const int r = root_of(key);
                K.set_node(j, k, r);
                slot = (uint32_t)r;
                bp = best_pack(key, k);
            }
            agg_atomics(s.ccnt, s.cbest, slot, bp);
        });
        __syncthreads();
        if (tid == 0) {
            int S = 0;
            for (int r = 0; r < nini; ++r) {
                if (s.ccnt[r] == 0) continue;
                QNode nd;
                nd.x0 = (int16_t)(int)__fmul_rn(g.hx, (float)r);
                nd.x1 = (int16_t)(int)__fmul_rn(g.hx, (float)(r + 1));
                nd.y0 = 0;
                nd.y1 = (int16_t)(g.h - 2 * kBorder);
                nd.count = (int32_t)s.ccnt[r];
                nd.best = s.cbest[r];
                nd.seq = 0;
                s.cur[S] = nd;
                s.nidx_s[r] = (int16_t)S;
                ++S;
            }
            sh_S = S;
        }
        __syncthreads();
        K.each([&](int j, int k) { K.set_node(j, k, s.nidx_s[K.node(j, k)]); });
        zero_children<NT>(s, sh_S);   // (the roots' counts were read before the barrier above)
        __syncthreads();
    }
    PHASE_MARK(2, 1);   // roots

    if (p.dbg_stop == 2) return;
    int S;
    if constexpr (NT == 256 && NR > 0) {
        // the 256-thread register path: a stats pass at the top of each round,
        // the move and the counters' zeroing after the node phase
        // (0.403 -> 0.395 ms per 3072 VGA frames against the one-pass rounds
        // below, profiles/r04_ab_qt_rounds_vga.txt)
        // ---- 3. full rounds (ORBextractor.cc:618-696)
        bool final_phase = false;
        if (pre_cnt)   // (roots counted in the gather: the keys move to the roots' list positions)
            K.each([&](int j, int k) { K.set_node(j, k, s.nidx_c[4 * K.node(j, k)]); });
        while (true) {
            const int S = sh_S;
            child_stats(s, K);
            PHASE_MARK(2, 2);   // full rounds: child counts
            // per node: (non-empty children | single-key parents << 21 | children
            // with more than one key << 42), scanned over a contiguous node range
            // per thread, so each thread reads back only its own entries
            const int per = (S + NT - 1) / NT;
            const int i0 = min(tid * per, S), i1 = min(i0 + per, S);
            uint64_t local = 0;
            for (int i = i0; i < i1; ++i) {
                uint64_t v = 1ull << 21;
                if (s.cur[i].count > 1) {
                    uint64_t nc = 0, ex = 0;
                    for (int q = 0; q < 4; ++q) { nc += s.ccnt[4 * i + q] > 0; ex += s.ccnt[4 * i + q] > 1; }
                    v = nc | (ex << 42);
                }
                s.a64[i] = v;
                local += v;
            }
            const uint64_t incl = wave_incl_scan_u64(local);
            if ((tid & 63) == 63) ws64[tid >> 6] = incl;
            __syncthreads();
            uint64_t run = incl - local, tot = 0;
            for (int w = 0; w < NT / 64; ++w) {
                if (w < (tid >> 6)) run += ws64[w];
                tot += ws64[w];
            }
            const int C = (int)(tot & 0x1FFFFF), singles = (int)((tot >> 21) & 0x1FFFFF);
            const int nexp = (int)(tot >> 42);
            const int S2 = C + singles;
            if (S2 > NC) {  // cannot happen by the bound in make_plan; fail loudly
                if (tid == 0) *level_count = -1;
                return;
            }
            for (int i = i0; i < i1; ++i) {
                const uint64_t pre = run;
                run += s.a64[i];
                const QNode nd = s.cur[i];
                if (nd.count > 1) {
                    int pos = (int)(pre & 0x1FFFFF);
                    for (int q = 0; q < 4; ++q) {
                        if (s.ccnt[4 * i + q] == 0) continue;
                        const int ni = C - 1 - pos;
                        s.nxt[ni] = make_child(s, nd, i, q, pos);
                        s.nidx_c[4 * i + q] = (int16_t)ni;
                        ++pos;
                    }
                } else {
                    const int ni = C + (int)((pre >> 21) & 0x1FFFFF);
                    s.nxt[ni] = nd;
                    set_all_quads(s.nidx_c, i, ni);
                }
            }
            __syncthreads();
            K.each([&](int j, int k) { K.set_node(j, k, s.nidx_c[4 * K.node(j, k) + K.quad(j, k)]); });
            zero_children<NT>(s, S2);
            {
                QNode *t = s.cur; s.cur = s.nxt; s.nxt = t;
            }
            if (tid == 0) sh_S = S2;
            __syncthreads();
            PHASE_MARK(2, 3);   // full rounds: scan + children
            if (S2 >= N || S2 == S) break;
            if (S2 + nexp * 3 > N) { final_phase = true; break; }
        }

        if (p.dbg_stop == 3) return;
        // ---- 4. final phase (ORBextractor.cc:697-762)
        while (final_phase) {
            const int S = sh_S;
            if (tid == 0) sh_nv = 0;   // (ordered by child_stats' barrier)
            child_stats(s, K);
            {
                int nz = 0;
                for (int i = tid; i < s.np2; i += NT) {
                    uint64_t v = 0;
                    if (i < S && s.cur[i].count > 1)
                        v = ((uint64_t)s.cur[i].count << 40) | ((uint64_t)s.cur[i].seq << 16) | (uint64_t)i;
                    s.a64[i] = v;
                    s.b64[i] = 0;
                    nz += v != 0;
                }
                nz = wave_sum_i32(nz);
                if ((tid & 63) == 0 && nz) atomicAdd(&sh_nv, nz);
            }
            for (int i = tid; i < S; i += NT) s.mark[i] = 0;
            __syncthreads();
            PHASE_MARK(2, 4);   // final: child counts
            // descending order of the splittable nodes' (count, seq, index) keys
            // (all distinct) by rank counting: one barrier instead of a bitonic
            // network's log^2 stages; zeros (unsplittable) stay behind, in b64
            {
                // eight entries per step, their four reads issued together (one LDS
                // round trip per step instead of per pair); a64[S, np2) is 0 and np2
                // a power of two >= 8
                const int S8 = (S + 7) & ~7;
                for (int i = tid; i < S; i += NT) {
                    const uint64_t v = s.a64[i];
                    if (v == 0) continue;
                    int r = 0;
                    for (int j = 0; j < S8; j += 8) {
                        const ulonglong2 w0 = *reinterpret_cast<const ulonglong2 *>(s.a64 + j);
                        const ulonglong2 w1 = *reinterpret_cast<const ulonglong2 *>(s.a64 + j + 2);
                        const ulonglong2 w2 = *reinterpret_cast<const ulonglong2 *>(s.a64 + j + 4);
                        const ulonglong2 w3 = *reinterpret_cast<const ulonglong2 *>(s.a64 + j + 6);
                        r += (w0.x > v) + (w0.y > v) + (w1.x > v) + (w1.y > v) + (w2.x > v) + (w2.y > v) +
                             (w3.x > v) + (w3.y > v);
                    }
                    s.b64[r] = v;
                }
                __syncthreads();
                uint64_t *t = s.a64; s.a64 = s.b64; s.b64 = t;
            }
            PHASE_MARK(2, 5);   // final: sort
            // per rank: number of non-empty children (nc) and gain (nc - 1)
            for (int r = tid; r < s.np2; r += NT) {
                uint64_t v = 0;
                if (s.a64[r] != 0) {
                    const int i = (int)(s.a64[r] & 0xFFFF);
                    int nc = 0;
                    for (int q = 0; q < 4; ++q) nc += s.ccnt[4 * i + q] > 0;
                    v = (uint64_t)nc | ((uint64_t)(nc - 1) << 32);
                }
                s.b64[r] = v;
            }
            if (tid == 0) sh_R = -1;
            __syncthreads();
            const int nv = sh_nv;
            block_excl_scan_u64<NT>(s.b64, s.np2, ws64);
            for (int r = tid; r < nv; r += NT) {
                const int i = (int)(s.a64[r] & 0xFFFF);
                int nc = 0;
                for (int q = 0; q < 4; ++q) nc += s.ccnt[4 * i + q] > 0;
                const int incl = (int)(s.b64[r] >> 32) + nc - 1;
                const int prev = (int)(s.b64[r] >> 32);
                if (S + incl >= N && S + prev < N) sh_R = r + 1;
            }
            __syncthreads();
            const int R = sh_R < 0 ? nv : sh_R;
            int CC;
            {
                if (R > 0) {
                    const int i = (int)(s.a64[R - 1] & 0xFFFF);
                    int nc = 0;
                    for (int q = 0; q < 4; ++q) nc += s.ccnt[4 * i + q] > 0;
                    CC = (int)(s.b64[R - 1] & 0xFFFFFFFF) + nc;
                } else {
                    CC = 0;
                }
            }
            const int S2 = CC + (S - R);
            if (S2 > NC) {
                if (tid == 0) *level_count = -1;
                return;
            }
            for (int r = tid; r < R; r += NT) {
                const int i = (int)(s.a64[r] & 0xFFFF);
                int cs = (int)(s.b64[r] & 0xFFFFFFFF);
                const QNode nd = s.cur[i];
                for (int q = 0; q < 4; ++q) {
                    if (s.ccnt[4 * i + q] == 0) continue;
                    const int ni = CC - 1 - cs;
                    s.nxt[ni] = make_child(s, nd, i, q, cs);
                    s.nidx_c[4 * i + q] = (int16_t)ni;
                    ++cs;
                }
                s.mark[i] = 1;
            }
            __syncthreads();
            for (int i = tid; i < s.np2; i += NT) s.b64[i] = (i < S && !s.mark[i]) ? 1 : 0;
            __syncthreads();
            block_excl_scan_u64<NT>(s.b64, s.np2, ws64);
            for (int i = tid; i < S; i += NT) {
                if (s.mark[i]) continue;
                const int ni = CC + (int)s.b64[i];
                s.nxt[ni] = s.cur[i];
                set_all_quads(s.nidx_c, i, ni);
            }
            __syncthreads();
            K.each([&](int j, int k) { K.set_node(j, k, s.nidx_c[4 * K.node(j, k) + K.quad(j, k)]); });
            zero_children<NT>(s, S2);
            {
                QNode *t = s.cur; s.cur = s.nxt; s.nxt = t;
            }
            if (tid == 0) sh_S = S2;
            __syncthreads();
            PHASE_MARK(2, 6);   // final: splits
            if (S2 >= N || S2 == S) break;
        }
        S = sh_S;
    } else {
        // Each round is one key pass: the pass that moves the keys into their
        // new nodes also adds them to those nodes' child counts (advance_stats),
        // and the child counts are re-zeroed in the round's node phase (each
        // thread its own nodes' entries after it read them, plus [4 S, 4 S2)), so
        // the rounds need no pass of their own for either.  The last round's move
        // only matters to the register path's output (phase 5).
        bool final_phase = false;
        S = sh_S;
        if (pre_cnt) advance_stats(s, K);
        else child_stats(s, K);
        PHASE_MARK(2, 2);   // child counts
        // ---- 3. full rounds (ORBextractor.cc:618-696)
        while (true) {
            // per node: (non-empty children | single-key parents << 21 | children
            // with more than one key << 42), scanned over a contiguous node range
            // per thread, so each thread reads back only its own entries
            const int per = (S + NT - 1) / NT;
            const int i0 = min(tid * per, S), i1 = min(i0 + per, S);
            uint64_t local = 0;
            for (int i = i0; i < i1; ++i) {
                uint64_t v = 1ull << 21;
                if (s.cur[i].count > 1) {
                    uint64_t nc = 0, ex = 0;
                    for (int q = 0; q < 4; ++q) { nc += s.ccnt[4 * i + q] > 0; ex += s.ccnt[4 * i + q] > 1; }
                    v = nc | (ex << 42);
                }
                s.a64[i] = v;
                local += v;
            }
            const uint64_t incl = wave_incl_scan_u64(local);
            if ((tid & 63) == 63) ws64[tid >> 6] = incl;
            __syncthreads();
            uint64_t run = incl - local, tot = 0;
            for (int w = 0; w < NT / 64; ++w) {
                if (w < (tid >> 6)) run += ws64[w];
                tot += ws64[w];
            }
            const int C = (int)(tot & 0x1FFFFF), singles = (int)((tot >> 21) & 0x1FFFFF);
            const int nexp = (int)(tot >> 42);
            const int S2 = C + singles;
            if (S2 > NC) {  // cannot happen by the bound in make_plan; fail loudly
                if (tid == 0) *level_count = -1;
                return;
            }
            for (int i = i0; i < i1; ++i) {
                const uint64_t pre = run;
                run += s.a64[i];
                const QNode nd = s.cur[i];
                if (nd.count > 1) {
                    int pos = (int)(pre & 0x1FFFFF);
                    for (int q = 0; q < 4; ++q) {
                        if (s.ccnt[4 * i + q] == 0) continue;
                        const int ni = C - 1 - pos;
                        s.nxt[ni] = make_child(s, nd, i, q, pos);
                        s.nidx_c[4 * i + q] = (int16_t)ni;
                        ++pos;
                    }
                } else {
                    const int ni = C + (int)((pre >> 21) & 0x1FFFFF);
                    s.nxt[ni] = nd;
                    set_all_quads(s.nidx_c, i, ni);
                }
            }
            // (only this thread reads its nodes' child entries)
            for (int i = 4 * i0; i < 4 * i1; ++i) { s.ccnt[i] = 0; s.cbest[i] = 0; }
            for (int i = 4 * S + tid; i < 4 * S2; i += NT) { s.ccnt[i] = 0; s.cbest[i] = 0; }
            __syncthreads();
            {
                QNode *t = s.cur; s.cur = s.nxt; s.nxt = t;
            }
            PHASE_MARK(2, 3);   // full rounds: scan + children
            const bool stop = S2 >= N || S2 == S;
            final_phase = !stop && S2 + nexp * 3 > N;
            S = S2;
            if (stop) {
                if constexpr (NR > 0) K.each([&](int j, int k) { K.set_node(j, k, s.nidx_c[4 * K.node(j, k) + K.quad(j, k)]); });
                break;
            }
            if (tid == 0) sh_nv = 0;   // (the final phase's count; ordered by the pass's barrier)
            advance_stats(s, K);
            PHASE_MARK(2, 2);   // full rounds: move + child counts
            if (final_phase) break;
        }

        if (p.dbg_stop == 3) return;
        // ---- 4. final phase (ORBextractor.cc:697-762); the child counts of the
        //         S nodes are in place
        while (final_phase) {
            {
                int nz = 0;
                for (int i = tid; i < s.np2; i += NT) {
                    uint64_t v = 0;
                    if (i < S && s.cur[i].count > 1)
                        v = ((uint64_t)s.cur[i].count << 40) | ((uint64_t)s.cur[i].seq << 16) | (uint64_t)i;
                    s.a64[i] = v;
                    s.b64[i] = 0;
                    nz += v != 0;
                }
                nz = wave_sum_i32(nz);
                if ((tid & 63) == 0 && nz) atomicAdd(&sh_nv, nz);
            }
            for (int i = tid; i < S; i += NT) s.mark[i] = 0;
            __syncthreads();
            PHASE_MARK(2, 4);   // final: node keys
            // descending order of the splittable nodes' (count, seq, index) keys
            // (all distinct) by rank counting: one barrier instead of a bitonic
            // network's log^2 stages; zeros (unsplittable) stay behind, in b64
            {
                // eight entries per step, their four reads issued together (one LDS
                // round trip per step instead of per pair); a64[S, np2) is 0 and np2
                // a power of two >= 8
                const int S8 = (S + 7) & ~7;
                for (int i = tid; i < S; i += NT) {
                    const uint64_t v = s.a64[i];
                    if (v == 0) continue;
                    int r = 0;
                    for (int j = 0; j < S8; j += 8) {
                        const ulonglong2 w0 = *reinterpret_cast<const ulonglong2 *>(s.a64 + j);
                        const ulonglong2 w1 = *reinterpret_cast<const ulonglong2 *>(s.a64 + j + 2);
                        const ulonglong2 w2 = *reinterpret_cast<const ulonglong2 *>(s.a64 + j + 4);
                        const ulonglong2 w3 = *reinterpret_cast<const ulonglong2 *>(s.a64 + j + 6);
                        r += (w0.x > v) + (w0.y > v) + (w1.x > v) + (w1.y > v) + (w2.x > v) + (w2.y > v) +
                             (w3.x > v) + (w3.y > v);
                    }
                    s.b64[r] = v;
                }
                __syncthreads();
                uint64_t *t = s.a64; s.a64 = s.b64; s.b64 = t;
            }
            PHASE_MARK(2, 5);   // final: sort
            // per rank: number of non-empty children (nc) and gain (nc - 1)
            for (int r = tid; r < s.np2; r += NT) {
                uint64_t v = 0;
                if (s.a64[r] != 0) {
                    const int i = (int)(s.a64[r] & 0xFFFF);
                    int nc = 0;
                    for (int q = 0; q < 4; ++q) nc += s.ccnt[4 * i + q] > 0;
                    v = (uint64_t)nc | ((uint64_t)(nc - 1) << 32);
                }
                s.b64[r] = v;
            }
            if (tid == 0) sh_R = -1;
            __syncthreads();
            const int nv = sh_nv;
            block_excl_scan_u64<NT>(s.b64, s.np2, ws64);
            for (int r = tid; r < nv; r += NT) {
                const int i = (int)(s.a64[r] & 0xFFFF);
                int nc = 0;
                for (int q = 0; q < 4; ++q) nc += s.ccnt[4 * i + q] > 0;
                const int incl = (int)(s.b64[r] >> 32) + nc - 1;
                const int prev = (int)(s.b64[r] >> 32);
                if (S + incl >= N && S + prev < N) sh_R = r + 1;
            }
            __syncthreads();
            const int R = sh_R < 0 ? nv : sh_R;
            int CC;
            {
                if (R > 0) {
                    const int i = (int)(s.a64[R - 1] & 0xFFFF);
                    int nc = 0;
                    for (int q = 0; q < 4; ++q) nc += s.ccnt[4 * i + q] > 0;
                    CC = (int)(s.b64[R - 1] & 0xFFFFFFFF) + nc;
                } else {
                    CC = 0;
                }
            }
            const int S2 = CC + (S - R);
            if (S2 > NC) {
                if (tid == 0) *level_count = -1;
                return;
            }
            for (int r = tid; r < R; r += NT) {
                const int i = (int)(s.a64[r] & 0xFFFF);
                int cs = (int)(s.b64[r] & 0xFFFFFFFF);
                const QNode nd = s.cur[i];
                for (int q = 0; q < 4; ++q) {
                    if (s.ccnt[4 * i + q] == 0) continue;
                    const int ni = CC - 1 - cs;
                    s.nxt[ni] = make_child(s, nd, i, q, cs);
                    s.nidx_c[4 * i + q] = (int16_t)ni;
                    ++cs;
                }
                s.mark[i] = 1;
            }
            __syncthreads();
            // (the child entries are read no more this round: re-zeroed for the
            // next round's counts, S2 >= S)
            for (int i = tid; i < s.np2; i += NT) s.b64[i] = (i < S && !s.mark[i]) ? 1 : 0;
            zero_children<NT>(s, S2);
            __syncthreads();
            block_excl_scan_u64<NT>(s.b64, s.np2, ws64);
            for (int i = tid; i < S; i += NT) {
                if (s.mark[i]) continue;
                const int ni = CC + (int)s.b64[i];
                s.nxt[ni] = s.cur[i];
                set_all_quads(s.nidx_c, i, ni);
            }
            __syncthreads();
            {
                QNode *t = s.cur; s.cur = s.nxt; s.nxt = t;
            }
            PHASE_MARK(2, 6);   // final: splits
            const bool stop = S2 >= N || S2 == S;
            S = S2;
            if (stop) {
                if constexpr (NR > 0) K.each([&](int j, int k) { K.set_node(j, k, s.nidx_c[4 * K.node(j, k) + K.quad(j, k)]); });
                break;
            }
            if (tid == 0) sh_nv = 0;
            advance_stats(s, K);
            PHASE_MARK(2, 4);   // final: move + child counts
        }
    }

    // ---- 5. best key per node, in list order (ORBextractor.cc:765-784)
    uint32_t *sel = fb.sel + (int64_t)b * p.out_cap + g.out_off;
    const int S_out = min(S, g.out_cap);
    if constexpr (NR > 0) {
        // the owner of each node's best key writes it (keys live in registers)
        K.each([&](int j, int k) {
            const int nd = K.node(j, k);
            if (nd < S_out && 0xFFFFFF - (int)(s.cur[nd].best & 0xFFFFFF) == k) sel[nd] = K.key[j];
        });
    } else {
        for (int i = tid; i < S_out; i += NT) {
            const int k = 0xFFFFFF - (int)(s.cur[i].best & 0xFFFFFF);
            sel[i] = keys[k];
        }
    }
    if (tid == 0) *level_count = S <= g.out_cap ? S : -1;
    PHASE_MARK(2, 7);   // output
}

template <bool PIPE, int NT>
__global__ __launch_bounds__(NT, QCfg<NT>::MINB) void k_quadtree(DevPlan p, FrameBufs fb, int l0) {
    extern __shared__ __align__(16) uint8_t lds[];
    PHASE_START();
    // (level-major grid: every frame's level 0, the longest, goes out first)
    const int l = l0 + blockIdx.y, b = blockIdx.x;
    const int tid = threadIdx.x;
    const LevelGeom g = p.lv[l];
    const int NC = p.node_cap;
    QLds s;
    s.np2 = 1;
    while (s.np2 < NC) s.np2 <<= 1;
    uint8_t *ptr = lds;
    s.a64 = reinterpret_cast<uint64_t *>(ptr); ptr += sizeof(uint64_t) * s.np2;
    s.b64 = reinterpret_cast<uint64_t *>(ptr); ptr += sizeof(uint64_t) * s.np2;
    s.cur = reinterpret_cast<QNode *>(ptr); ptr += sizeof(QNode) * NC;
    s.nxt = reinterpret_cast<QNode *>(ptr); ptr += sizeof(QNode) * NC;
    s.ccnt = reinterpret_cast<uint32_t *>(ptr); ptr += sizeof(uint32_t) * 4 * NC;
    s.cbest = reinterpret_cast<uint32_t *>(ptr); ptr += sizeof(uint32_t) * 4 * NC;
    s.nidx_c = reinterpret_cast<int16_t *>(ptr); ptr += sizeof(int16_t) * 4 * NC;
    s.nidx_s = reinterpret_cast<int16_t *>(ptr); ptr += sizeof(int16_t) * NC;
    s.mark = ptr;

    const int64_t kbase = (int64_t)b * p.cand_cap + g.cand_off;
    uint32_t *keys = fb.keys + kbase;
    uint16_t *knode = fb.key_node + kbase;
    uint8_t *kq = fb.key_q + kbase;
    int32_t *level_count = fb.level_count + (int64_t)b * kMaxLevels + l;

    // ---- 1. gather the level's candidates in cell order (the order the
    //         reference pushes them into vToDistributeKeys): per-cell start
    //         offsets and sources in LDS (the node arrays are free until phase 2)
    const int ncell = g.cell_end - g.cell_begin;
    int *cell_off = reinterpret_cast<int *>(lds);            // ncell + 1
    int *cell_src = cell_off + ncell + 1;                    // slot | bit 31: minThFAST list
    // key k's source (slot index | bit 31: minThFAST list), for the first
    // QCfg<NT>::KR keys: each cell's thread writes its keys' entries right after
    // the scan, so the keys load with one LDS read each after one barrier
    uint32_t *kaddr = reinterpret_cast<uint32_t *>(cell_src + ncell);
    __shared__ int ws2[2 * (NT / 64)];   // scan partials, alternating per chunk
    int base = 0;
    for (int c0 = 0, chunk = 0; c0 < ncell; c0 += NT, ++chunk) {
        const int c = c0 + tid;
        int word = 0, slot = 0;
        if (c < ncell) {
            word = fb.cell_count[(int64_t)b * p.ncells + g.cell_begin + c];
            slot = p.cells[g.cell_begin + c].slot;
        }
        const int cnt = word & 0x7FFFFFFF;
        int *ws = ws2 + (chunk & 1) * (NT / 64);
        const int incl = wave_incl_scan_i32(cnt);
        if ((tid & 63) == 63) ws[tid >> 6] = incl;
        __syncthreads();
        int pre = 0, tot = 0;
        for (int w = 0; w < NT / 64; ++w) {
            if (w < (tid >> 6)) pre += ws[w];
            tot += ws[w];
        }
        if (c < ncell) {
            const int off = base + pre + incl - cnt;
            const uint32_t src = (uint32_t)slot | (word < 0 ? 0x80000000u : 0u);
            cell_off[c] = off;
            cell_src[c] = (int)src;
            for (int i = 0; i < cnt && off + i < QCfg<NT>::KR; ++i) kaddr[off + i] = src + (uint32_t)i;
        }
        base += tot;
    }
    const int n = base;
    if (tid == 0) cell_off[ncell] = n;
    __syncthreads();
    if (p.dbg_stop == 1) return;
    if (n == 0 || g.nini <= 0) {
        if (tid == 0) *level_count = 0;
        return;
    }
    const uint32_t *cand = fb.cand + (int64_t)b * p.cand_cap, *cand2 = fb.cand2 + (int64_t)b * p.cand_cap;
    // the roots counted in the gather when there are few (every level but the
    // narrowest strips; one root has its own pass without atomics): count and
    // best key per root by the aggregated atomics, each key's node = its root
    // and quadrant 0 set with it (no roots pass over the keys of its own)
    __shared__ uint32_t rcnt[kQPreRoots], rbest[kQPreRoots];
    const int nini = g.nini;
    auto root_of = [&](uint32_t key) {
        const float rx = (float)((int)(key & 0xFFF) - kBorder);
        return min((int)__fdiv_rn(rx, g.hx), nini - 1);
    };
    // up to QCfg<NT>::R1 (R2) keys per thread stay in registers
    // through the rounds
    auto in_registers = [&](auto &K) {
        K.gkeys = nullptr; K.gnode = knode; K.gq = kq; K.n = n;
        K.each([&](int j, int k) {
            const uint32_t a = kaddr[k];
            K.key[j] = ((int)a < 0 ? cand2 : cand)[a & 0x7FFFFFFFu];
            K.nq[j] = 0;
        });
        __syncthreads();   // the cell tables are dead from here
        PHASE_MARK(2, 0);   // gather
        quadtree_rounds(p, fb, s, g, b, l, K, phase_t_);
    };
    if (n <= QCfg<NT>::R1 * NT) {
        QKeys<QCfg<NT>::R1, NT> K;
        in_registers(K);
    } else if (n <= QCfg<NT>::R2 * NT) {
        QKeys<QCfg<NT>::R2, NT> K;
        in_registers(K);
    } else {
        QKeys<0, NT> K;
        K.gkeys = keys; K.gnode = knode; K.gq = kq; K.n = n;
        // the cell of key 64 m for every m (in the key-source map's LDS,
        // unused on this path): a wave's 64 keys (k0 is a multiple of 64)
        // then bisect only the cells between two of them
        const int nco = (n + 63) >> 6;
        int *coarse = reinterpret_cast<int *>(kaddr);
        const bool use_co = nco < QCfg<NT>::KR;
        if (use_co) {
            for (int c = tid; c < ncell; c += NT) {
                const int o = cell_off[c], e = cell_off[c + 1];
                for (int m = (o + 63) >> 6; (m << 6) < e; ++m) coarse[m] = c;
            }
            if (tid == 0) coarse[nco] = ncell - 1;
        }
        // the roots counted here when there are few (rcnt / rbest above)
        const bool pre = nini <= kQPreRoots;
        if (tid < kQPreRoots) { rcnt[tid] = 0; rbest[tid] = 0; }
        __syncthreads();
        // kQU keys per thread at a time (the chunk mapping of QKeys<0>): their
        // bisections interleave, and their candidate loads go out together
        for (int k0 = 0; k0 < n; k0 += NT * kQU) {
            int lo[kQU], hi[kQU];
#pragma unroll
            for (int u = 0; u < kQU; ++u) {
                const int m = (k0 + u * NT + tid) >> 6;   // (wave-uniform)
                lo[u] = use_co && m < nco ? coarse[m] : 0;
                hi[u] = use_co && m < nco ? coarse[m + 1] : ncell - 1;
            }
            for (bool more = true; more;) {
                more = false;
#pragma unroll
                for (int u = 0; u < kQU; ++u) {
                    const int k = k0 + u * NT + tid;
                    if (lo[u] < hi[u]) {
                        const int mid = (lo[u] + hi[u] + 1) >> 1;
                        if (cell_off[mid] <= k) lo[u] = mid; else hi[u] = mid - 1;
                        more |= lo[u] < hi[u];
                    }
                }
            }
#pragma unroll
            for (int u = 0; u < kQU; ++u) {
                const int k = k0 + u * NT + tid;
                uint32_t slot = ~0u, bp = 0;
                if (k < n) {
                    const int src = cell_src[lo[u]];
                    const uint32_t key = ((src < 0) ? cand2 : cand)[(src & 0x7FFFFFFF) + (k - cell_off[lo[u]])];
                    keys[k] = key;
                    if (pre) {
                        int r = 0;
                        if (nini > 1) r = root_of(key);
                        knode[k] = (uint16_t)r;
                        kq[k] = 0;
                        slot = (uint32_t)r;
                        bp = best_pack(key, k);
                    }
                }
                if (pre) agg_atomics(rcnt, rbest, slot, bp);   // (every lane: DPP)
            }
        }
        __syncthreads();
        PHASE_MARK(2, 0);
        if (pre) quadtree_rounds(p, fb, s, g, b, l, K, phase_t_, rcnt, rbest);
        else quadtree_rounds(p, fb, s, g, b, l, K, phase_t_);
    }
}

}  // namespace

// Workgroup size of k_quadtree for a launch of `blocks` (level, frame)
// blocks: 1024 threads when the launch is too small to fill the chip with
// 256-thread workgroups (a few frames: the drop-in call, a sharded camera
// set); 512 for images of more than 0.6 MP (HD, FHD: thousands of keys on
// every level, up to 20 per thread in registers, two workgroups per CU);
// else 256 (VGA: <= 8 register keys per thread, 7 workgroups per CU).
// ORBX_QT_NT=256 / 512 / 1024 forces one (where its LDS fits); ORBX_QT_WIDE=0
// never takes 1024, =1 always (read per launch: tests switch them per extractor).
int quadtree_nt(const DevPlan &p, int blocks) {
    const bool wide_fits = p.node_lds_bytes_w <= 160 * 1024;
    if (const char *e = std::getenv("ORBX_QT_NT")) {
        const int nt = std::atoi(e);
        if ((nt == 512 || nt == 1024) && wide_fits) return nt;
        if (nt == 256) return 256;
    }
    const char *w = std::getenv("ORBX_QT_WIDE");
    const int mode = w ? std::atoi(w) : -1;
    if (!wide_fits) return 256;
    if (mode == 1 || (mode != 0 && blocks <= 256)) return 1024;
    return (int64_t)p.lv[0].w * p.lv[0].h > 600 * 1000 ? 512 : 256;
}

template <bool PIPE>
hipError_t launch_quadtree_range(const DevPlan &p, const FrameBufs &fb, int B, hipStream_t st, int l, int l_end) {
    const dim3 grid(B, l_end - l);   // level-major: workgroups go out level by level (longest first), not frame by frame
    switch (quadtree_nt(p, (l_end - l) * B)) {
        case 1024:
            if (allow_lds(k_quadtree<PIPE, 1024>, p.node_lds_bytes_w) != hipSuccess) return hipErrorInvalidValue;
            hipLaunchKernelGGL((k_quadtree<PIPE, 1024>), grid, dim3(1024), p.node_lds_bytes_w, st, p, fb, l);
            break;
        case 512:
            if (allow_lds(k_quadtree<PIPE, 512>, p.node_lds_bytes_w) != hipSuccess) return hipErrorInvalidValue;
            hipLaunchKernelGGL((k_quadtree<PIPE, 512>), grid, dim3(512), p.node_lds_bytes_w, st, p, fb, l);
            break;
        default:
            if (allow_lds(k_quadtree<PIPE, kThreads>, p.node_lds_bytes) != hipSuccess) return hipErrorInvalidValue;
            hipLaunchKernelGGL((k_quadtree<PIPE, kThreads>), grid, dim3(kThreads), p.node_lds_bytes, st, p, fb, l);
    }
    return hipGetLastError();
}

hipError_t launch_quadtree(const DevPlan &p, const FrameBufs &fb, int B, hipStream_t st) {
    return launch_quadtree_range<false>(p, fb, B, st, 0, p.nlevels);
}

hipError_t launch_quadtree_level(const DevPlan &p, const FrameBufs &fb, int B, hipStream_t st, int l, int l_end) {
    return launch_quadtree_range<true>(p, fb, B, st, l, l_end);
}

int quadtree_lds_bytes(int node_cap) {
    int np2 = 1;
    while (np2 < node_cap) np2 <<= 1;
    return (int)(2 * sizeof(uint64_t) * np2 + 2 * sizeof(QNode) * node_cap +
                 2 * sizeof(uint32_t) * 4 * node_cap + sizeof(int16_t) * 5 * node_cap + node_cap + 64);
}

}  // namespace orbx
