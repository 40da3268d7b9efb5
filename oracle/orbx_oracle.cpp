/*
 * orbx_oracle.cpp -- CPU restatement of ORB-SLAM2's ORBextractor / ORBmatcher
 * hot path, used ONLY as the parity checker and the CPU baseline.
 *
 * TEST INFRASTRUCTURE.  Parity vs the reference binary: UNPINNED (see
 * orbx_oracle.h).  Every function cites the reference line range it restates.
 * Compile with -ffp-contract=off: the reference (CMake Release, no -march,
 * CMakeLists.txt:4-6) runs on x86-64 SSE2 without FMA contraction.
 *
 * Written as an independent formulation from the HIP kernels: this file follows
 * the reference's sequential structure (FAST three-row buffers, std::list
 * quadtree, per-keypoint loops); the kernels use per-pixel arc scores,
 * round-synchronous node arrays and wave ballots.
 */
#include "orbx_oracle.h"

#include <algorithm>
#include <atomic>
#include <cfloat>
#include <climits>
#include <cmath>
#include <cstring>
#include <list>
#include <map>
#include <set>
#include <unordered_map>
#include <vector>

namespace {

// ---------------------------------------------------------------------------
// OpenCV 3.2 scalar helpers (x86-64): cvRound = cvtss2si/cvtsd2si (half-even).
// ---------------------------------------------------------------------------
inline int cv_round(float v) { return (int)std::nearbyint(v); }
inline int cv_round(double v) { return (int)std::nearbyint(v); }
inline int cv_floor(float v) { int i = cv_round(v); return i - (float(i) > v ? 1 : 0); }
inline int cv_floor(double v) { int i = cv_round(v); return i - (double(i) > v ? 1 : 0); }
inline int cv_ceil(double v) { int i = cv_round(v); return i + (double(i) < v ? 1 : 0); }
inline short sat_short(float v) {
    int i = cv_round(v);
    return (short)std::min(std::max(i, (int)SHRT_MIN), (int)SHRT_MAX);
}
inline uint8_t sat_u8(int v) { return (uint8_t)std::min(std::max(v, 0), 255); }
inline int16_t sat_s16(int v) { return (int16_t)std::min(std::max(v, -32768), 32767); }

// cv::fastAtan2, OpenCV 3.2 core/src/mathfuncs_core.cpp (degrees in [0,360)).
const float kAtanP1 = 0.9997878412794807f * (float)(180 / M_PI);
const float kAtanP3 = -0.3258083974640975f * (float)(180 / M_PI);
const float kAtanP5 = 0.1555786518463281f * (float)(180 / M_PI);
const float kAtanP7 = -0.04432655554792128f * (float)(180 / M_PI);

float fast_atan2(float y, float x) {
    float ax = std::fabs(x), ay = std::fabs(y), a, c, c2;
    if (ax >= ay) {
        c = ay / (ax + (float)DBL_EPSILON);
        c2 = c * c;
        a = (((kAtanP7 * c2 + kAtanP5) * c2 + kAtanP3) * c2 + kAtanP1) * c;
    } else {
        c = ax / (ay + (float)DBL_EPSILON);
        c2 = c * c;
        a = 90.f - (((kAtanP7 * c2 + kAtanP5) * c2 + kAtanP3) * c2 + kAtanP1) * c;
    }
    if (x < 0) a = 180.f - a;
    if (y < 0) a = 360.f - a;
    return a;
}

int reflect101(int p, int len) {
    if (len == 1) return 0;
    while (p < 0 || p >= len) p = p < 0 ? -p : 2 * len - p - 2;
    return p;
}

// ---------------------------------------------------------------------------
// cv::resize(src, dst, dsize, 0, 0, INTER_LINEAR) for 8UC1, OpenCV 3.2:
// coefficient tables (resize(), imgwarp.cpp), HResizeLinear<uchar,int,short>
// and VResizeLinear with the SSE2 VResizeLinearVec_32s8u body for the leading
// columns and the FixedPtCast<int,uchar,22> scalar tail.
// Reference call site: ORBextractor.cc:1171.
// ---------------------------------------------------------------------------
void resize_linear(const uint8_t *src, int sw, int sh, size_t sstep,
                   uint8_t *dst, int dw, int dh, size_t dstep) {
    const double inv_sx = (double)dw / sw, inv_sy = (double)dh / sh;
    const double scale_x = 1. / inv_sx, scale_y = 1. / inv_sy;
    std::vector<int> xofs(dw);
    std::vector<short> ialpha(2 * dw);
    int xmax = dw;
    for (int dx = 0; dx < dw; ++dx) {
        float fx = (float)((dx + 0.5) * scale_x - 0.5);
        int sx = cv_floor(fx);
        fx -= sx;
        if (sx < 0) { fx = 0.f; sx = 0; }
        if (sx + 1 >= sw) {
            xmax = std::min(xmax, dx);
            if (sx >= sw - 1) { fx = 0.f; sx = sw - 1; }
        }
        xofs[dx] = sx;
        ialpha[2 * dx] = sat_short((1.f - fx) * 2048);
        ialpha[2 * dx + 1] = sat_short(fx * 2048);
    }
    // SSE2 vertical pass covers [0, xs); the scalar loop the rest.
    int xs = 0;
    while (xs <= dw - 16) xs += 16;
    while (xs < dw - 4) xs += 4;

    std::vector<int> h0(dw), h1(dw);
    auto hrow = [&](int r, std::vector<int> &h) {
        const uint8_t *S = src + (size_t)r * sstep;
        for (int dx = 0; dx < dw; ++dx) {
            int sx = xofs[dx];
            h[dx] = dx < xmax ? S[sx] * ialpha[2 * dx] + S[sx + 1] * ialpha[2 * dx + 1]
                              : S[sx] * 2048;
        }
    };
    for (int dy = 0; dy < dh; ++dy) {
        float fy = (float)((dy + 0.5) * scale_y - 0.5);
        int sy = cv_floor(fy);
        fy -= sy;
        const short b0 = sat_short((1.f - fy) * 2048), b1 = sat_short(fy * 2048);
        const int r0 = std::min(std::max(sy, 0), sh - 1);
        const int r1 = std::min(std::max(sy + 1, 0), sh - 1);
        hrow(r0, h0);
        hrow(r1, h1);
        uint8_t *D = dst + (size_t)dy * dstep;
        for (int x = 0; x < dw; ++x) {
            if (x < xs) {
                // _mm_packs_epi32(srai 4) -> _mm_mulhi_epi16 -> _mm_adds_epi16 -> (+2)>>2 -> packus
                int16_t a = sat_s16(h0[x] >> 4), b = sat_s16(h1[x] >> 4);
                int16_t p = (int16_t)((a * (int)b0) >> 16), q = (int16_t)((b * (int)b1) >> 16);
                int16_t s = sat_s16(p + q);
                s = sat_s16(s + 2);
                D[x] = sat_u8(s >> 2);
            } else {
                D[x] = sat_u8((h0[x] * b0 + h1[x] * b1 + (1 << 21)) >> 22);
            }
        }
    }
}

// ---------------------------------------------------------------------------
// cv::GaussianBlur(img, img, Size(7,7), 2, 2, BORDER_REFLECT_101) for 8UC1,
// OpenCV 3.2: getGaussianKernel(7, 2, CV_32F) -> fixed-point separable filter
// (createSeparableLinearFilter: kernels x256 -> int, bits 16): integer row
// pass, SymmColumnVec_32s8u (SSE2, float accumulation + cvtps rounding) on the
// leading 4*floor(w/4) columns, FixedPtCastEx<int,uchar>(16) scalar tail.
// Reference call site: ORBextractor.cc:1129-1130.
// ---------------------------------------------------------------------------
void gauss_kernel_int(int k[7]) {
    float cf[7];
    double sum = 0;
    const double sigma = 2.0, scale2X = -0.5 / (sigma * sigma);
    for (int i = 0; i < 7; ++i) {
        double x = i - 3.0;
        cf[i] = (float)std::exp(scale2X * x * x);
        sum += cf[i];
    }
    sum = 1. / sum;
    for (int i = 0; i < 7; ++i) cf[i] = (float)(cf[i] * sum);
    for (int i = 0; i < 7; ++i) k[i] = cv_round(cf[i] * 256.f);
}

void gauss7(const uint8_t *src, int w, int h, size_t sstep, uint8_t *dst, size_t dstep) {
    int k[7];
    gauss_kernel_int(k);
    float kf[4];
    for (int i = 0; i < 4; ++i) kf[i] = (float)k[3 + i] * (1.f / 65536.f);
    // Row pass into an int image (exact).
    std::vector<int> R((size_t)w * h);
    for (int y = 0; y < h; ++y) {
        const uint8_t *S = src + (size_t)y * sstep;
        for (int x = 0; x < w; ++x) {
            int acc = 0;
            for (int t = 0; t < 7; ++t) acc += k[t] * S[reflect101(x + t - 3, w)];
            R[(size_t)y * w + x] = acc;
        }
    }
    const int xs = w & ~3;
    for (int y = 0; y < h; ++y) {
        const int *row[7];
        for (int t = 0; t < 7; ++t) row[t] = &R[(size_t)reflect101(y + t - 3, h) * w];
        uint8_t *D = dst + (size_t)y * dstep;
        for (int x = 0; x < w; ++x) {
            if (x < xs) {
                float s = (float)row[3][x] * kf[0] + 0.f;
                for (int t = 1; t <= 3; ++t)
                    s = s + (float)(row[3 + t][x] + row[3 - t][x]) * kf[t];
                int v = (int)std::nearbyint(s);  // cvtps_epi32
                D[x] = sat_u8(sat_s16(v));
            } else {
                int s = k[3] * row[3][x];
                for (int t = 1; t <= 3; ++t) s += k[3 + t] * (row[3 + t][x] + row[3 - t][x]);
                D[x] = sat_u8((s + (1 << 15)) >> 16);
            }
        }
    }
}

// ---------------------------------------------------------------------------
// cv::FAST(img, kps, th, nonmax=true), TYPE_9_16, OpenCV 3.2 features2d/src/
// fast.cpp FAST_t<16> + fast_score.cpp cornerScore<16>.  Restated with the
// three-row score buffers of the original; output order row-major.
// Reference call sites: ORBextractor.cc:842, 848.
// ---------------------------------------------------------------------------
const int kCircle[16][2] = {{0, 3}, {1, 3}, {2, 2}, {3, 1}, {3, 0}, {3, -1}, {2, -2}, {1, -3},
                            {0, -3}, {-1, -3}, {-2, -2}, {-3, -1}, {-3, 0}, {-3, 1}, {-2, 2}, {-1, 3}};

int corner_score16(const uint8_t *p, const int off[25], int threshold) {
    int v = p[0], d[25];
    for (int k = 0; k < 25; ++k) d[k] = v - p[off[k]];
    int a0 = threshold;
    for (int k = 0; k < 16; k += 2) {
        int a = std::min(d[k + 1], d[k + 2]);
        a = std::min(a, d[k + 3]);
        if (a <= a0) continue;
        for (int t = 4; t <= 8; ++t) a = std::min(a, d[k + t]);
        a0 = std::max(a0, std::min(a, d[k]));
        a0 = std::max(a0, std::min(a, d[k + 9]));
    }
    int b0 = -a0;
    for (int k = 0; k < 16; k += 2) {
        int b = std::max(d[k + 1], d[k + 2]);
        b = std::max(b, d[k + 3]);
        b = std::max(b, d[k + 4]);
        b = std::max(b, d[k + 5]);
        if (b >= b0) continue;
        for (int t = 6; t <= 8; ++t) b = std::max(b, d[k + t]);
        b0 = std::min(b0, std::max(b, d[k]));
        b0 = std::min(b0, std::max(b, d[k + 9]));
    }
    return -b0 - 1;
}

struct Corner { int x, y, score; };

void fast9(const uint8_t *img, int w, int h, size_t step, int threshold, std::vector<Corner> &out) {
    out.clear();
    threshold = std::min(std::max(threshold, 0), 255);
    int off[25];
    for (int k = 0; k < 16; ++k) off[k] = kCircle[k][0] + kCircle[k][1] * (int)step;
    for (int k = 16; k < 25; ++k) off[k] = off[k - 16];
    uint8_t tab[512];
    for (int i = -255; i <= 255; ++i)
        tab[i + 255] = (uint8_t)(i < -threshold ? 1 : i > threshold ? 2 : 0);
    std::vector<uint8_t> sbuf(3 * (size_t)std::max(w, 1), 0);
    std::vector<int> cpos[3];
    for (int i = 3; i < h - 2; ++i) {
        uint8_t *curr = &sbuf[(size_t)((i - 3) % 3) * w];
        std::vector<int> &cp = cpos[(i - 3) % 3];
        std::memset(curr, 0, w);
        cp.clear();
        if (i < h - 3) {
            for (int j = 3; j < w - 3; ++j) {
                const uint8_t *p = img + (size_t)i * step + j;
                const int v = p[0];
                const uint8_t *t = &tab[255 - v];
                int d = t[p[off[0]]] | t[p[off[8]]];
                if (!d) continue;
                d &= t[p[off[2]]] | t[p[off[10]]];
                d &= t[p[off[4]]] | t[p[off[12]]];
                d &= t[p[off[6]]] | t[p[off[14]]];
                if (!d) continue;
                d &= t[p[off[1]]] | t[p[off[9]]];
                d &= t[p[off[3]]] | t[p[off[11]]];
                d &= t[p[off[5]]] | t[p[off[13]]];
                d &= t[p[off[7]]] | t[p[off[15]]];
                for (int pass = 0; pass < 2; ++pass) {
                    if (!(d & (1 << pass))) continue;
                    int run = 0;
                    for (int k = 0; k < 25; ++k) {
                        int x = p[off[k]];
                        bool hit = pass == 0 ? x < v - threshold : x > v + threshold;
                        if (!hit) { run = 0; continue; }
                        if (++run > 8) {
                            cp.push_back(j);
                            curr[j] = (uint8_t)corner_score16(p, off, threshold);
                            break;
                        }
                    }
                }
            }
        }
        if (i == 3) continue;
        const uint8_t *prev = &sbuf[(size_t)((i - 4 + 3) % 3) * w];
        const uint8_t *pprev = &sbuf[(size_t)((i - 5 + 3) % 3) * w];
        for (int j : cpos[(i - 4 + 3) % 3]) {
            int s = prev[j];
            if (s > prev[j + 1] && s > prev[j - 1] && s > pprev[j - 1] && s > pprev[j] &&
                s > pprev[j + 1] && s > curr[j - 1] && s > curr[j] && s > curr[j + 1])
                out.push_back({j, i - 1, s});
        }
    }
}

// ---------------------------------------------------------------------------
// ORBextractor constructor tables (ORBextractor.cc:416-479).
// ---------------------------------------------------------------------------
struct Geometry {
    int nlevels;
    std::vector<float> scale, inv_scale;
    std::vector<int> w, h, quota;
    int umax[16];
};

Geometry make_geometry(int W, int H, int nfeatures, float scaleFactorF, int nlevels) {
    Geometry g;
    g.nlevels = nlevels;
    const double scaleFactor = scaleFactorF;  // member is double (ORBextractor.h:98)
    g.scale.assign(nlevels, 1.f);
    for (int i = 1; i < nlevels; ++i) g.scale[i] = (float)(g.scale[i - 1] * scaleFactor);
    g.inv_scale.resize(nlevels);
    for (int i = 0; i < nlevels; ++i) g.inv_scale[i] = 1.0f / g.scale[i];
    g.quota.assign(nlevels, 0);
    float factor = (float)(1.0f / scaleFactor);
    float nDesired = nfeatures * (1 - factor) / (1 - (float)std::pow((double)factor, (double)nlevels));
    int sum = 0;
    for (int l = 0; l < nlevels - 1; ++l) {
        g.quota[l] = cv_round(nDesired);
        sum += g.quota[l];
        nDesired *= factor;
    }
    g.quota[nlevels - 1] = std::max(nfeatures - sum, 0);
    g.w.resize(nlevels);
    g.h.resize(nlevels);
    for (int l = 0; l < nlevels; ++l) {
        g.w[l] = cv_round((float)W * g.inv_scale[l]);
        g.h[l] = cv_round((float)H * g.inv_scale[l]);
    }
    // umax (ORBextractor.cc:463-478)
    const int HP = 15;
    int vmax = cv_floor(HP * std::sqrt(2.f) / 2 + 1);
    int vmin = cv_ceil(HP * std::sqrt(2.f) / 2);
    const double hp2 = HP * HP;
    for (int v = 0; v <= vmax; ++v) g.umax[v] = cv_round(std::sqrt(hp2 - v * v));
    for (int v = HP, v0 = 0; v >= vmin; --v) {
        while (g.umax[v0] == g.umax[v0 + 1]) ++v0;
        g.umax[v] = v0;
        ++v0;
    }
    return g;
}

// ---------------------------------------------------------------------------
// Cell loop of ComputeKeyPointsOctTree (ORBextractor.cc:796-863).
// ---------------------------------------------------------------------------
// The sub-images cv::FAST is called on, [x0, x1) x [y0, y1) in level pixels,
// in the reference's visiting order (skipped cells left out).
struct CellWin { int x0, y0, x1, y1; };

void level_cells(int w, int h, std::vector<CellWin> &cells) {
    cells.clear();
    const float W = 30;
    const int minBX = 19 - 3, minBY = minBX;
    const int maxBX = w - 19 + 3, maxBY = h - 19 + 3;
    const float width = (float)(maxBX - minBX), height = (float)(maxBY - minBY);
    const int nCols = (int)(width / W), nRows = (int)(height / W);
    if (nCols <= 0 || nRows <= 0) return;
    const int wCell = (int)std::ceil(width / nCols), hCell = (int)std::ceil(height / nRows);
    for (int i = 0; i < nRows; ++i) {
        const float iniY = (float)(minBY + i * hCell);
        float maxY = iniY + hCell + 6;
        if (iniY >= maxBY - 3) continue;
        if (maxY > maxBY) maxY = (float)maxBY;
        for (int j = 0; j < nCols; ++j) {
            const float iniX = (float)(minBX + j * wCell);
            float maxX = iniX + wCell + 6;
            if (iniX >= maxBX - 6) continue;
            if (maxX > maxBX) maxX = (float)maxBX;
            cells.push_back({(int)iniX, (int)iniY, (int)maxX, (int)maxY});
        }
    }
}

void level_candidates(const uint8_t *lvl, int w, int h, size_t step, int iniTh, int minTh,
                      std::vector<Corner> &cands, std::vector<int> *cell_counts = nullptr) {
    cands.clear();
    if (cell_counts) cell_counts->clear();
    std::vector<CellWin> cells;
    level_cells(w, h, cells);
    std::vector<Corner> cell;
    for (const CellWin &cw : cells) {
        const int x0 = cw.x0, y0 = cw.y0;
        const uint8_t *sub = lvl + (size_t)y0 * step + x0;
        const int sw = cw.x1 - x0, sh = cw.y1 - y0;
        fast9(sub, sw, sh, step, iniTh, cell);
        if (cell.empty()) fast9(sub, sw, sh, step, minTh, cell);
        for (const Corner &c : cell) cands.push_back({c.x + x0, c.y + y0, c.score});
        if (cell_counts) cell_counts->push_back((int)cell.size());
    }
}

// ---------------------------------------------------------------------------
// DistributeOctTree (ORBextractor.cc:561-787) + ExtractorNode::DivideNode
// (ORBextractor.cc:498-554), restated on std::list with the reference's
// push_front / erase order.  The reference sorts (size, ExtractorNode*) pairs
// (:705-708), i.e. breaks size ties by heap address; this restatement breaks
// them by creation number (later-created == larger address), documented in
// DESIGN.md §3.4.
// Coordinates are relative to (minBorderX, minBorderY) = (16, 16).
// ---------------------------------------------------------------------------
struct QNode {
    int x0, y0, x1, y1;
    std::vector<int> keys;
    bool no_more = false;
    long seq = 0;
    std::list<QNode>::iterator self;
};

void divide(const QNode &p, const std::vector<Corner> &c, QNode ch[4]) {
    const int hx = (int)std::ceil((float)(p.x1 - p.x0) / 2);
    const int hy = (int)std::ceil((float)(p.y1 - p.y0) / 2);
    const int mx = p.x0 + hx, my = p.y0 + hy;
    ch[0].x0 = p.x0; ch[0].y0 = p.y0; ch[0].x1 = mx;   ch[0].y1 = my;
    ch[1].x0 = mx;   ch[1].y0 = p.y0; ch[1].x1 = p.x1; ch[1].y1 = my;
    ch[2].x0 = p.x0; ch[2].y0 = my;   ch[2].x1 = mx;   ch[2].y1 = p.y1;
    ch[3].x0 = mx;   ch[3].y0 = my;   ch[3].x1 = p.x1; ch[3].y1 = p.y1;
    for (int q = 0; q < 4; ++q) ch[q].keys.clear();
    for (int k : p.keys) {
        const int x = c[k].x - 16, y = c[k].y - 16;
        int q = (x < mx) ? (y < my ? 0 : 2) : (y < my ? 1 : 3);
        ch[q].keys.push_back(k);
    }
    for (int q = 0; q < 4; ++q) ch[q].no_more = ch[q].keys.size() == 1;
}

// Diagnostic (tools/tie_exposure.py): how often the reference's pointer tie
// rule could matter.  [0] levels, [1] levels with a final phase, [2] final
// rounds, [3] rounds splitting >= 2 equal-size nodes (their children's list
// order follows the tie rule), [4] nodes in those groups, [5] rounds whose
// cutoff falls inside a group of equal-size nodes (which of them are split
// follows the tie rule), [6] nodes in those groups, [7] levels with [3] or
// [5], [8] levels with [5].
static std::atomic<long> g_tie[9];   // (the CPU baseline runs the oracle on many threads)
// Tie order of the final-phase sort: 0 creation order (the restatement's rule),
// 1 reverse creation order, k >= 2 a seeded pseudo-random order -- other heap
// layouts the reference could meet (diagnostic only: tools/tie_exposure.py).
static std::atomic<int> g_tie_mode{0};
static inline unsigned long tie_key(long seq, int mode) {
    if (mode == 0) return (unsigned long)seq;
    if (mode == 1) return ~(unsigned long)seq;
    unsigned long z = (unsigned long)seq * 0x9E3779B97F4A7C15ull + (unsigned long)mode * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 31)) * 0x94D049BB133111EBull;
    return z ^ (z >> 29);
}

std::vector<int> distribute(const std::vector<Corner> &c, int w, int h, int N) {
    ++g_tie[0];
    bool lv_any = false, lv_set = false, lv_final = false;
    const int minX = 16, maxX = w - 16, minY = 16, maxY = h - 16;
    std::vector<int> result;
    if (c.empty()) return result;
    const int nIni = (int)std::round((float)(maxX - minX) / (maxY - minY));
    const float hX = (float)(maxX - minX) / nIni;
    long seq = 0;
    std::list<QNode> L;
    std::vector<QNode *> ini(nIni);
    for (int i = 0; i < nIni; ++i) {
        QNode n;
        n.x0 = (int)(hX * (float)i);
        n.x1 = (int)(hX * (float)(i + 1));
        n.y0 = 0;
        n.y1 = maxY - minY;
        n.seq = seq++;
        L.push_back(n);
        ini[i] = &L.back();
    }
    for (size_t k = 0; k < c.size(); ++k) {
        const float x = (float)(c[k].x - 16);
        ini[(size_t)(x / hX)]->keys.push_back((int)k);
    }
    for (auto it = L.begin(); it != L.end();) {
        if (it->keys.size() == 1) { it->no_more = true; ++it; }
        else if (it->keys.empty()) it = L.erase(it);
        else ++it;
    }

    struct Expand { int size; long seq; QNode *node; };
    std::vector<Expand> expand;
    auto push_children = [&](QNode ch[4], bool count_expand, int *nToExpand) {
        for (int q = 0; q < 4; ++q) {
            if (ch[q].keys.empty()) continue;
            ch[q].seq = seq++;
            L.push_front(ch[q]);
            if (ch[q].keys.size() > 1) {
                if (count_expand) ++*nToExpand;
                expand.push_back({(int)ch[q].keys.size(), ch[q].seq, &L.front()});
                L.front().self = L.begin();
            }
        }
    };

    bool finish = false;
    while (!finish) {
        const int prevSize = (int)L.size();
        int nToExpand = 0;
        expand.clear();
        for (auto it = L.begin(); it != L.end();) {
            if (it->no_more) { ++it; continue; }
            QNode ch[4];
            divide(*it, c, ch);
            push_children(ch, true, &nToExpand);
            it = L.erase(it);
        }
        if ((int)L.size() >= N || (int)L.size() == prevSize) {
            finish = true;
        } else if ((int)L.size() + nToExpand * 3 > N) {
            while (!finish) {
                const int prev = (int)L.size();
                std::vector<Expand> todo = expand;
                expand.clear();
                const int tm = g_tie_mode.load(std::memory_order_relaxed);
                std::sort(todo.begin(), todo.end(), [tm](const Expand &a, const Expand &b) {
                    return a.size != b.size ? a.size < b.size : tie_key(a.seq, tm) < tie_key(b.seq, tm);
                });
                int jb = 0;   // lowest split index
                for (int j = (int)todo.size() - 1; j >= 0; --j) {
                    QNode ch[4];
                    divide(*todo[j].node, c, ch);
                    push_children(ch, false, nullptr);
                    L.erase(todo[j].node->self);
                    jb = j;
                    if ((int)L.size() >= N) break;
                }
                if (!lv_final) { lv_final = true; ++g_tie[1]; }
                ++g_tie[2];
                {   // tie groups among the split nodes todo[jb..]
                    bool ord = false;
                    long ord_nodes = 0;
                    for (int a = jb; a < (int)todo.size();) {
                        int e = a;
                        while (e + 1 < (int)todo.size() && todo[e + 1].size == todo[a].size) ++e;
                        const int lo = std::max(a, jb);
                        if (e - lo + 1 >= 2) { ord = true; ord_nodes += e - lo + 1; }
                        a = e + 1;
                    }
                    if (ord) { ++g_tie[3]; g_tie[4] += ord_nodes; lv_any = true; }
                    if (jb > 0 && todo[jb - 1].size == todo[jb].size) {
                        int a = jb, e = jb;
                        while (a > 0 && todo[a - 1].size == todo[jb].size) --a;
                        while (e + 1 < (int)todo.size() && todo[e + 1].size == todo[jb].size) ++e;
                        ++g_tie[5];
                        g_tie[6] += e - a + 1;
                        lv_any = lv_set = true;
                    }
                }
                if ((int)L.size() >= N || (int)L.size() == prev) finish = true;
            }
        }
    }
    if (lv_any) ++g_tie[7];
    if (lv_set) ++g_tie[8];
    for (const QNode &n : L) {
        int best = n.keys[0];
        for (size_t k = 1; k < n.keys.size(); ++k)
            if (c[n.keys[k]].score > c[best].score) best = n.keys[k];
        result.push_back(best);
    }
    return result;
}

// IC_Angle (ORBextractor.cc:77-104) on the unblurred level.
float ic_angle(const uint8_t *lvl, size_t step, int x, int y, const int umax[16]) {
    const uint8_t *center = lvl + (size_t)y * step + x;
    int m01 = 0, m10 = 0;
    for (int u = -15; u <= 15; ++u) m10 += u * center[u];
    for (int v = 1; v <= 15; ++v) {
        int vsum = 0;
        const int d = umax[v];
        for (int u = -d; u <= d; ++u) {
            const int plus = center[u + v * (int)step], minus = center[u - v * (int)step];
            vsum += plus - minus;
            m10 += u * (plus + minus);
        }
        m01 += v * vsum;
    }
    return fast_atan2((float)m01, (float)m10);
}

const int8_t kPattern[512][2] = {
#define ORBX_PATTERN_BEGIN
#define ORBX_PATTERN_END
#include "../orb_slam_2_ros_amd/csrc/orb_pattern.inc"
#undef ORBX_PATTERN_BEGIN
#undef ORBX_PATTERN_END
};

// computeOrbDescriptor (ORBextractor.cc:106-147) on the blurred level.
void orb_descriptor(const uint8_t *blur, size_t step, int x, int y, float angle_deg, uint8_t *desc) {
    const float factorPI = (float)(M_PI / 180.f);
    const float angle = angle_deg * factorPI;
    const float a = (float)std::cos(angle), b = (float)std::sin(angle);
    const uint8_t *center = blur + (size_t)y * step + x;
    auto sample = [&](int idx) {
        const float px = (float)kPattern[idx][0], py = (float)kPattern[idx][1];
        const int r = cv_round(px * b + py * a);
        const int col = cv_round(px * a - py * b);
        return (int)center[r * (int)step + col];
    };
    for (int i = 0; i < 32; ++i) {
        int val = 0;
        for (int k = 0; k < 8; ++k) {
            const int p = 16 * i + 2 * k;
            val |= (sample(p) < sample(p + 1)) << k;
        }
        desc[i] = (uint8_t)val;
    }
}

int hamming32(const uint8_t *a, const uint8_t *b) {
    int dist = 0;
    for (int i = 0; i < 8; ++i) {
        uint32_t pa, pb;
        std::memcpy(&pa, a + 4 * i, 4);
        std::memcpy(&pb, b + 4 * i, 4);
        uint32_t v = pa ^ pb;
        v = v - ((v >> 1) & 0x55555555u);
        v = (v & 0x33333333u) + ((v >> 2) & 0x33333333u);
        dist += (int)((((v + (v >> 4)) & 0xF0F0F0Fu) * 0x1010101u) >> 24);
    }
    return dist;
}

struct Pyramid {
    std::vector<std::vector<uint8_t>> lv;
};

Pyramid build_pyramid(const uint8_t *img, int W, int H, size_t step, const Geometry &g) {
    Pyramid p;
    p.lv.resize(g.nlevels);
    p.lv[0].resize((size_t)W * H);
    for (int y = 0; y < H; ++y) std::memcpy(&p.lv[0][(size_t)y * W], img + (size_t)y * step, W);
    for (int l = 1; l < g.nlevels; ++l) {
        p.lv[l].resize((size_t)g.w[l] * g.h[l]);
        resize_linear(p.lv[l - 1].data(), g.w[l - 1], g.h[l - 1], g.w[l - 1],
                      p.lv[l].data(), g.w[l], g.h[l], g.w[l]);
    }
    return p;
}

}  // namespace

// =============================================================================
extern "C" {

int orbo_cv_round(float v) { return cv_round(v); }
float orbo_fast_atan2(float y, float x) { return fast_atan2(y, x); }
void orbo_sincosf(float a, float *s, float *c) { *c = (float)std::cos(a); *s = (float)std::sin(a); }
int orbo_descriptor_distance(const uint8_t *a, const uint8_t *b) { return hamming32(a, b); }

void orbo_resize_linear(const uint8_t *src, int sw, int sh, size_t sstep,
                        uint8_t *dst, int dw, int dh, size_t dstep) {
    resize_linear(src, sw, sh, sstep, dst, dw, dh, dstep);
}

void orbo_gauss7(const uint8_t *src, int w, int h, size_t sstep, uint8_t *dst, size_t dstep) {
    gauss7(src, w, h, sstep, dst, dstep);
}

int orbo_fast(const uint8_t *img, int w, int h, size_t step, int threshold, int32_t *xys, int cap) {
    std::vector<Corner> out;
    fast9(img, w, h, step, threshold, out);
    int n = (int)out.size();
    for (int i = 0; i < n && i < cap; ++i) {
        xys[3 * i] = out[i].x; xys[3 * i + 1] = out[i].y; xys[3 * i + 2] = out[i].score;
    }
    return n;
}

void orbo_levels(int w, int h, int nfeatures, float scaleFactor, int nlevels,
                 int *lw, int *lh, int *quota, float *scale) {
    Geometry g = make_geometry(w, h, nfeatures, scaleFactor, nlevels);
    for (int l = 0; l < nlevels; ++l) {
        lw[l] = g.w[l]; lh[l] = g.h[l]; quota[l] = g.quota[l]; scale[l] = g.scale[l];
    }
}

size_t orbo_pyramid(const uint8_t *img, int w, int h, size_t step, float scaleFactor, int nlevels,
                    uint8_t *out) {
    Geometry g = make_geometry(w, h, 1000, scaleFactor, nlevels);
    Pyramid p = build_pyramid(img, w, h, step, g);
    size_t off = 0;
    for (int l = 0; l < nlevels; ++l) {
        std::memcpy(out + off, p.lv[l].data(), p.lv[l].size());
        off += p.lv[l].size();
    }
    return off;
}

int orbo_level_candidates(const uint8_t *lvl, int w, int h, int iniTh, int minTh,
                          int32_t *xys, int cap) {
    std::vector<Corner> c;
    level_candidates(lvl, w, h, w, iniTh, minTh, c);
    const int n = (int)c.size();
    if (n > cap) return -n;
    for (int i = 0; i < n; ++i) {
        xys[3 * i] = c[i].x; xys[3 * i + 1] = c[i].y; xys[3 * i + 2] = c[i].score;
    }
    return n;
}

// The same with the corner count of every visited cell, in the reference's
// cell order (tools/tie_heap: the per-cell vector<KeyPoint> allocations).
// Returns the candidate count, or -(count) if cap or cell_cap is too small.
int orbo_level_candidates_cells(const uint8_t *lvl, int w, int h, int iniTh, int minTh, int32_t *xys, int cap,
                                int32_t *cell_counts, int cell_cap, int *ncells) {
    std::vector<Corner> c;
    std::vector<int> cc;
    level_candidates(lvl, w, h, w, iniTh, minTh, c, &cc);
    const int n = (int)c.size();
    *ncells = (int)cc.size();
    if (n > cap || (int)cc.size() > cell_cap) return -n;
    for (int i = 0; i < n; ++i) {
        xys[3 * i] = c[i].x; xys[3 * i + 1] = c[i].y; xys[3 * i + 2] = c[i].score;
    }
    for (size_t i = 0; i < cc.size(); ++i) cell_counts[i] = cc[i];
    return n;
}

// The FAST sub-image windows (x0, y0, x1, y1) of a w x h level, in the same
// cell order.  Returns the cell count, or -(count) if cap is too small.
int orbo_level_cells(int w, int h, int32_t *rects, int cap) {
    std::vector<CellWin> cells;
    level_cells(w, h, cells);
    const int n = (int)cells.size();
    if (n > cap) return -n;
    for (int i = 0; i < n; ++i) {
        rects[4 * i] = cells[i].x0; rects[4 * i + 1] = cells[i].y0;
        rects[4 * i + 2] = cells[i].x1; rects[4 * i + 3] = cells[i].y1;
    }
    return n;
}

void orbo_set_tie_mode(int mode) { g_tie_mode = mode; }

void orbo_tie_stats(int64_t out[9], int reset) {
    for (int i = 0; i < 9; ++i) out[i] = reset ? g_tie[i].exchange(0) : g_tie[i].load();
}

int orbo_distribute(const int32_t *xys, int n, int w, int h, int N, int32_t *sel) {
    std::vector<Corner> c(n);
    for (int i = 0; i < n; ++i) c[i] = {xys[3 * i], xys[3 * i + 1], xys[3 * i + 2]};
    std::vector<int> r = distribute(c, w, h, N);
    for (size_t i = 0; i < r.size(); ++i) sel[i] = r[i];
    return (int)r.size();
}

int orbo_extract(const uint8_t *img, int w, int h, size_t step,
                 int nfeatures, float scaleFactor, int nlevels, int iniTh, int minTh,
                 orbo_keypoint *kps, uint8_t *desc, int cap, int *n_out) {
    *n_out = 0;
    if (!img || w <= 0 || h <= 0) return 0;  // empty image: outputs untouched (:1086-1087)
    Geometry g = make_geometry(w, h, nfeatures, scaleFactor, nlevels);
    Pyramid p = build_pyramid(img, w, h, step, g);
    struct LevelOut { std::vector<Corner> keys; std::vector<float> ang; };
    std::vector<LevelOut> lo(nlevels);
    int total = 0;
    std::vector<Corner> cands;
    for (int l = 0; l < nlevels; ++l) {
        level_candidates(p.lv[l].data(), g.w[l], g.h[l], g.w[l], iniTh, minTh, cands);
        std::vector<int> sel = distribute(cands, g.w[l], g.h[l], g.quota[l]);
        for (int s : sel) lo[l].keys.push_back(cands[s]);
        for (const Corner &k : lo[l].keys) lo[l].ang.push_back(ic_angle(p.lv[l].data(), g.w[l], k.x, k.y, g.umax));
        total += (int)sel.size();
    }
    *n_out = total;
    if (total > cap) return -1;
    int o = 0;
    std::vector<uint8_t> blur;
    for (int l = 0; l < nlevels; ++l) {
        if (lo[l].keys.empty()) continue;
        blur.resize((size_t)g.w[l] * g.h[l]);
        gauss7(p.lv[l].data(), g.w[l], g.h[l], g.w[l], blur.data(), g.w[l]);
        const float size = (float)(int)(31 * g.scale[l]);
        for (size_t i = 0; i < lo[l].keys.size(); ++i, ++o) {
            const Corner &k = lo[l].keys[i];
            orb_descriptor(blur.data(), g.w[l], k.x, k.y, lo[l].ang[i], desc + 32 * (size_t)o);
            orbo_keypoint &kp = kps[o];
            kp.x = (float)k.x; kp.y = (float)k.y;
            if (l != 0) { kp.x *= g.scale[l]; kp.y *= g.scale[l]; }
            kp.size = size;
            kp.angle = lo[l].ang[i];
            kp.response = (float)k.score;
            kp.octave = l;
            kp.class_id = -1;
        }
    }
    return 0;
}

// SearchForInitialization (ORBmatcher.cc:406-521) with Frame grid semantics
// (Frame.cc:239-256 AssignFeaturesToGrid, :354-412 GetFeaturesInArea,
// :415-425 PosInGrid) and ComputeThreeMaxima (ORBmatcher.cc:1603-1644).
int orbo_search_for_initialization(const orbo_keypoint *k1, const uint8_t *d1, int n1,
                                   const orbo_keypoint *k2, const uint8_t *d2, int n2,
                                   int img_w, int img_h, float *prev_xy, int32_t *m12,
                                   int window, float nnratio, int check_ori) {
    return orbo_search_for_initialization_bounds(k1, d1, n1, k2, d2, n2, 0.f, (float)img_w, 0.f, (float)img_h,
                                                 prev_xy, m12, window, nnratio, check_ori);
}

// The grid over the Frame's image bounds (static mnMinX .. mnMaxY, Frame.cc:475-499).
int orbo_search_for_initialization_bounds(const orbo_keypoint *k1, const uint8_t *d1, int n1,
                                          const orbo_keypoint *k2, const uint8_t *d2, int n2,
                                          float minX, float maxX, float minY, float maxY, float *prev_xy,
                                          int32_t *m12, int window, float nnratio, int check_ori) {
    const int GC = 64, GR = 48, HL = 30, TH_LOW = 50;
    const float invW = (float)GC / (maxX - minX), invH = (float)GR / (maxY - minY);
    std::vector<std::vector<int>> grid((size_t)GC * GR);
    for (int i = 0; i < n2; ++i) {
        const int px = (int)std::round((k2[i].x - minX) * invW);
        const int py = (int)std::round((k2[i].y - minY) * invH);
        if (px < 0 || px >= GC || py < 0 || py >= GR) continue;
        grid[(size_t)px * GR + py].push_back(i);
    }
    for (int i = 0; i < n1; ++i) m12[i] = -1;
    std::vector<int> rot[HL];
    const float factor = 1.0f / HL;
    std::vector<int> matchedDist(n2, INT_MAX), m21(n2, -1);
    int nmatches = 0;
    const float r = (float)window;
    std::vector<int> cand;
    for (int i1 = 0; i1 < n1; ++i1) {
        if (k1[i1].octave > 0) continue;
        const float x = prev_xy[2 * i1], y = prev_xy[2 * i1 + 1];
        cand.clear();
        const int cx0 = std::max(0, (int)std::floor((x - minX - r) * invW));
        const int cx1 = std::min(GC - 1, (int)std::ceil((x - minX + r) * invW));
        const int cy0 = std::max(0, (int)std::floor((y - minY - r) * invH));
        const int cy1 = std::min(GR - 1, (int)std::ceil((y - minY + r) * invH));
        if (cx0 < GC && cx1 >= 0 && cy0 < GR && cy1 >= 0) {
            for (int ix = cx0; ix <= cx1; ++ix)
                for (int iy = cy0; iy <= cy1; ++iy)
                    for (int j : grid[(size_t)ix * GR + iy]) {
                        if (k2[j].octave < 0 || k2[j].octave > 0) continue;
                        if (std::fabs(k2[j].x - x) < r && std::fabs(k2[j].y - y) < r) cand.push_back(j);
                    }
        }
        if (cand.empty()) continue;
        int best = INT_MAX, best2 = INT_MAX, bestIdx = -1;
        for (int i2 : cand) {
            const int dist = hamming32(d1 + 32 * (size_t)i1, d2 + 32 * (size_t)i2);
            if (matchedDist[i2] <= dist) continue;
            if (dist < best) { best2 = best; best = dist; bestIdx = i2; }
            else if (dist < best2) best2 = dist;
        }
        if (best <= TH_LOW && best < (float)best2 * nnratio) {
            if (m21[bestIdx] >= 0) { m12[m21[bestIdx]] = -1; --nmatches; }
            m12[i1] = bestIdx;
            m21[bestIdx] = i1;
            matchedDist[bestIdx] = best;
            ++nmatches;
            if (check_ori) {
                float rotv = k1[i1].angle - k2[bestIdx].angle;
                if (rotv < 0.0) rotv += 360.0f;
                int bin = (int)std::round(rotv * factor);
                if (bin == HL) bin = 0;
                rot[bin].push_back(i1);
            }
        }
    }
    if (check_ori) {
        int max1 = 0, max2 = 0, max3 = 0, ind1 = -1, ind2 = -1, ind3 = -1;
        for (int i = 0; i < HL; ++i) {
            const int s = (int)rot[i].size();
            if (s > max1) { max3 = max2; max2 = max1; max1 = s; ind3 = ind2; ind2 = ind1; ind1 = i; }
            else if (s > max2) { max3 = max2; max2 = s; ind3 = ind2; ind2 = i; }
            else if (s > max3) { max3 = s; ind3 = i; }
        }
        if (max2 < 0.1f * (float)max1) { ind2 = -1; ind3 = -1; }
        else if (max3 < 0.1f * (float)max1) ind3 = -1;
        for (int i = 0; i < HL; ++i) {
            if (i == ind1 || i == ind2 || i == ind3) continue;
            for (int idx1 : rot[i])
                if (m12[idx1] >= 0) { m12[idx1] = -1; --nmatches; }
        }
    }
    for (int i1 = 0; i1 < n1; ++i1)
        if (m12[i1] >= 0) {
            prev_xy[2 * i1] = k2[m12[i1]].x;
            prev_xy[2 * i1 + 1] = k2[m12[i1]].y;
        }
    return nmatches;
}

}  // extern "C"

// Frame::ComputeStereoMatches (Frame.cc:502-676).  Row table Frame.cc:512-529,
// band search :540-585, SAD window + parabola :587-660, median cut :662-675.
// Where the reference has undefined behaviour or raises cv::Exception (row
// table or row index out of range; an SAD window outside the level, which
// Mat::rowRange/colRange assert on) this restatement reports "no match" for
// that keypoint; the product kernel does the same.
int orbo_compute_stereo_matches(const uint8_t *pyrL, const uint8_t *pyrR, const int *lw, const int *lh,
                                int nlevels, const float *scale, const float *inv_scale,
                                const orbo_keypoint *kl, const uint8_t *dl, int nl,
                                const orbo_keypoint *kr, const uint8_t *dr, int nr,
                                float mbf, float mb, float *uright, float *depth) {
    std::vector<size_t> off(nlevels + 1, 0);
    for (int l = 0; l < nlevels; ++l) off[l + 1] = off[l] + (size_t)lw[l] * lh[l];
    for (int i = 0; i < nl; ++i) { uright[i] = -1.0f; depth[i] = -1.0f; }
    const int TH_HIGH = 100, TH_LOW = 50, thOrbDist = (TH_HIGH + TH_LOW) / 2;
    const int nRows = lh[0];
    std::vector<std::vector<int>> rows(nRows);
    for (int iR = 0; iR < nr; ++iR) {
        const float y = kr[iR].y;
        const float r = 2.0f * scale[kr[iR].octave];
        const int maxr = (int)std::ceil(y + r), minr = (int)std::floor(y - r);
        for (int yi = minr; yi <= maxr; ++yi)
            if (yi >= 0 && yi < nRows) rows[yi].push_back(iR);
    }
    const float minZ = mb, minD = 0.f, maxD = mbf / minZ;
    std::vector<std::pair<int, int>> distIdx;
    for (int iL = 0; iL < nl; ++iL) {
        const orbo_keypoint &kL = kl[iL];
        const int levelL = kL.octave;
        const float vL = kL.y, uL = kL.x;
        if (!(vL >= 0.f) || vL >= (float)nRows) continue;
        const std::vector<int> &cands = rows[(size_t)vL];
        if (cands.empty()) continue;
        const float minU = uL - maxD, maxU = uL - minD;
        if (maxU < 0) continue;
        int bestDist = TH_HIGH;
        int bestIdxR = 0;
        for (int iR : cands) {
            if (kr[iR].octave < levelL - 1 || kr[iR].octave > levelL + 1) continue;
            const float uR = kr[iR].x;
            if (uR >= minU && uR <= maxU) {
                const int dist = hamming32(dl + 32 * (size_t)iL, dr + 32 * (size_t)iR);
                if (dist < bestDist) { bestDist = dist; bestIdxR = iR; }
            }
        }
        if (bestDist >= thOrbDist) continue;
        const float uR0 = kr[bestIdxR].x;
        const float sf = inv_scale[levelL];
        const float suL = std::round(uL * sf), svL = std::round(vL * sf), suR0 = std::round(uR0 * sf);
        const int W = 5, L = 5;
        const int cols = lw[levelL], nrows = lh[levelL];
        const int r0 = (int)(svL - W), cL0 = (int)(suL - W);
        if (svL - W < 0 || svL + W + 1 > nrows || suL - W < 0 || suL + W + 1 > cols) continue;  // cv assert
        const float iniu = suR0 + L - W, endu = suR0 + L + W + 1;
        if (iniu < 0 || endu >= cols) continue;
        if (suR0 - L - W < 0) continue;                                                        // cv assert
        const uint8_t *IL = pyrL + off[levelL], *IR = pyrR + off[levelL];
        const int cR0 = (int)suR0;
        const float cl = (float)IL[(size_t)(r0 + W) * cols + cL0 + W];
        int bestSad = INT_MAX, bestInc = 0;
        float dists[2 * L + 1];
        for (int inc = -L; inc <= L; ++inc) {
            const int c0 = cR0 + inc - W;
            const float cr = (float)IR[(size_t)(r0 + W) * cols + c0 + W];
            double acc = 0;   // cv::norm(NORM_L1) of CV_32F accumulates in double
            for (int r = 0; r < 2 * W + 1; ++r)
                for (int c = 0; c < 2 * W + 1; ++c) {
                    const float a = (float)IL[(size_t)(r0 + r) * cols + cL0 + c] - cl;
                    const float b = (float)IR[(size_t)(r0 + r) * cols + c0 + c] - cr;
                    acc += std::fabs((double)a - (double)b);
                }
            const float dist = (float)acc;
            if (dist < (float)bestSad) { bestSad = (int)dist; bestInc = inc; }
            dists[L + inc] = dist;
        }
        if (bestInc == -L || bestInc == L) continue;
        const float d1 = dists[L + bestInc - 1], d2 = dists[L + bestInc], d3 = dists[L + bestInc + 1];
        const float deltaR = (d1 - d3) / (2.0f * (d1 + d3 - 2.0f * d2));
        if (deltaR < -1 || deltaR > 1) continue;
        float bestuR = scale[levelL] * ((float)suR0 + (float)bestInc + deltaR);
        float disparity = uL - bestuR;
        if (disparity >= minD && disparity < maxD) {
            if (disparity <= 0) {
                disparity = 0.01;
                bestuR = uL - 0.01;
            }
            depth[iL] = mbf / disparity;
            uright[iL] = bestuR;
            distIdx.push_back(std::make_pair(bestSad, iL));
        }
    }
    if (distIdx.empty()) return 0;   // the reference reads distIdx[0] of an empty vector here
    std::sort(distIdx.begin(), distIdx.end());
    const float median = (float)distIdx[distIdx.size() / 2].first;
    const float thDist = 1.5f * 1.4f * median;
    int kept = (int)distIdx.size();
    for (int i = (int)distIdx.size() - 1; i >= 0; --i) {
        if ((float)distIdx[i].first < thDist) break;
        uright[distIdx[i].second] = -1;
        depth[distIdx[i].second] = -1;
        --kept;
    }
    return kept;
}

// Frame::ComputeStereoFromRGBD (Frame.cc:679-701): depth looked up at the
// (truncated) distorted keypoint, uRight from the undistorted one.
void orbo_stereo_from_rgbd(const orbo_keypoint *kps, const orbo_keypoint *kps_un, int n, const float *dmap,
                           int w, int h, size_t pitch_bytes, float mbf, float *uright, float *depth) {
    for (int i = 0; i < n; ++i) {
        uright[i] = -1; depth[i] = -1;
        const int v = (int)kps[i].y, u = (int)kps[i].x;
        if (v < 0 || v >= h || u < 0 || u >= w) continue;   // reference: unchecked Mat::at
        const float d = *(const float *)((const uint8_t *)dmap + (size_t)v * pitch_bytes + 4 * (size_t)u);
        if (d > 0) {
            depth[i] = d;
            uright[i] = kps_un[i].x - mbf / d;
        }
    }
}

// ---- projection matchers (ORBmatcher::SearchByProjection x4, Fuse x2 search) ----
namespace {

// Frame / KeyFrame 64x48 feature grid (Frame.cc:239-256, 415-425).
struct FeatureGrid {
    static constexpr int GC = 64, GR = 48;
    float minX, minY, invW, invH;
    std::vector<std::vector<int>> cells;
    FeatureGrid(const orbo_keypoint *k, int n, float min_x, float max_x, float min_y, float max_y)
        : minX(min_x), minY(min_y), invW((float)GC / (max_x - min_x)), invH((float)GR / (max_y - min_y)),
          cells((size_t)GC * GR) {
        for (int i = 0; i < n; ++i) {
            const int px = (int)std::round((k[i].x - minX) * invW);
            const int py = (int)std::round((k[i].y - minY) * invH);
            if (px < 0 || px >= GC || py < 0 || py >= GR) continue;
            cells[(size_t)px * GR + py].push_back(i);
        }
    }
    // Frame::GetFeaturesInArea (Frame.cc:354-412); KeyFrame's (KeyFrame.cc:700-739)
    // is the same walk without the level filter (minLevel = maxLevel = -1 here).
    std::vector<int> area(const orbo_keypoint *k, float x, float y, float r, int minLevel, int maxLevel) const {
        std::vector<int> out;
        const int nMinCellX = std::max(0, (int)std::floor((x - minX - r) * invW));
        if (nMinCellX >= GC) return out;
        const int nMaxCellX = std::min(GC - 1, (int)std::ceil((x - minX + r) * invW));
        if (nMaxCellX < 0) return out;
        const int nMinCellY = std::max(0, (int)std::floor((y - minY - r) * invH));
        if (nMinCellY >= GR) return out;
        const int nMaxCellY = std::min(GR - 1, (int)std::ceil((y - minY + r) * invH));
        if (nMaxCellY < 0) return out;
        const bool bCheckLevels = (minLevel > 0) || (maxLevel >= 0);
        for (int ix = nMinCellX; ix <= nMaxCellX; ix++)
            for (int iy = nMinCellY; iy <= nMaxCellY; iy++)
                for (int j : cells[(size_t)ix * GR + iy]) {
                    if (bCheckLevels) {
                        if (k[j].octave < minLevel) continue;
                        if (maxLevel >= 0 && k[j].octave > maxLevel) continue;
                    }
                    const float distx = k[j].x - x, disty = k[j].y - y;
                    if (std::fabs(distx) < r && std::fabs(disty) < r) out.push_back(j);
                }
        return out;
    }
};

// ComputeThreeMaxima (ORBmatcher.cc:1603-1644) on bin sizes.
void three_maxima(const int *sizes, int L, int &ind1, int &ind2, int &ind3) {
    int max1 = 0, max2 = 0, max3 = 0;
    ind1 = ind2 = ind3 = -1;
    for (int i = 0; i < L; i++) {
        const int s = sizes[i];
        if (s > max1) { max3 = max2; max2 = max1; max1 = s; ind3 = ind2; ind2 = ind1; ind1 = i; }
        else if (s > max2) { max3 = max2; max2 = s; ind3 = ind2; ind2 = i; }
        else if (s > max3) { max3 = s; ind3 = i; }
    }
    if (max2 < 0.1f * (float)max1) { ind2 = -1; ind3 = -1; }
    else if (max3 < 0.1f * (float)max1) { ind3 = -1; }
}

}  // namespace

int orbo_search_by_projection(int variant, const orbo_keypoint *keys, const uint8_t *desc, const float *uright,
                              const uint8_t *mp_state, const float *inv_sigma2, int n, float min_x, float max_x,
                              float min_y, float max_y, const orbo_proj_query *q, const uint8_t *qdesc, int nq,
                              int th_dist, float nnratio, int check_ori, int32_t *q_idx, int32_t *q_dist,
                              int32_t *kp_final) {
    const FeatureGrid grid(keys, n, min_x, max_x, min_y, max_y);
    const int HL = 30;
    const float factor = 1.0f / HL;
    std::vector<int> rotHist[HL];   // accepted queries per bin (the reference keeps their keypoints)
    // mvpMapPoints as (non-NULL, Observations() > 0) and which query put it there
    std::vector<uint8_t> has(n), obs(n);
    for (int i = 0; i < n; ++i) { has[i] = mp_state ? (mp_state[i] & 1) : 0; obs[i] = mp_state ? ((mp_state[i] >> 1) & 1) : 0; }
    for (int i = 0; i < n; ++i) kp_final[i] = -1;
    int nmatches = 0;
    for (int iq = 0; iq < nq; ++iq) {
        q_idx[iq] = -1;
        q_dist[iq] = -1;
        const orbo_proj_query &Q = q[iq];
        if (!(Q.flags & 1)) continue;
        const uint8_t *dq = qdesc + 32 * (size_t)iq;
        const std::vector<int> cand = grid.area(keys, Q.u, Q.v, Q.radius, Q.min_level, Q.max_level);
        if (cand.empty()) continue;
        if (variant == ORBO_PROJ_LOCALMAP) {
            // ORBmatcher.cc:45-129
            int bestDist = 256, bestLevel = -1, bestDist2 = 256, bestLevel2 = -1, bestIdx = -1;
            for (int idx : cand) {
                if (has[idx] && obs[idx]) continue;
                if (uright && uright[idx] > 0) {
                    const float er = std::fabs(Q.ur - uright[idx]);
                    if (er > Q.ur_tol) continue;
                }
                const int dist = hamming32(dq, desc + 32 * (size_t)idx);
                if (dist < bestDist) {
                    bestDist2 = bestDist; bestDist = dist;
                    bestLevel2 = bestLevel; bestLevel = keys[idx].octave;
                    bestIdx = idx;
                } else if (dist < bestDist2) {
                    bestLevel2 = keys[idx].octave; bestDist2 = dist;
                }
            }
            if (bestDist <= th_dist) {
                if (bestLevel == bestLevel2 && bestDist > nnratio * bestDist2) continue;
                has[bestIdx] = 1; obs[bestIdx] = (Q.flags >> 1) & 1;
                kp_final[bestIdx] = iq;
                q_idx[iq] = bestIdx; q_dist[iq] = bestDist;
                nmatches++;
            }
            continue;
        }
        // best-only variants
        const bool fuse = variant == ORBO_PROJ_FUSE || variant == ORBO_PROJ_FUSE_SIM3;
        int bestDist = variant == ORBO_PROJ_FUSE_SIM3 ? INT_MAX : 256, bestIdx = -1;
        for (int idx : cand) {
            if (variant == ORBO_PROJ_LASTFRAME) {             // ORBmatcher.cc:1403-1413
                if (has[idx] && obs[idx]) continue;
                if (uright && uright[idx] > 0) {
                    const float er = std::fabs(Q.ur - uright[idx]);
                    if (er > Q.ur_tol) continue;
                }
            } else if (variant == ORBO_PROJ_KEYFRAME || variant == ORBO_PROJ_SIM3) {   // :1546-1548, :371-372
                if (has[idx]) continue;
            } else if (variant == ORBO_PROJ_FUSE) {           // :903-932
                const orbo_keypoint &kp = keys[idx];
                const int kpLevel = kp.octave;
                if (uright && uright[idx] >= 0) {
                    const float ex = Q.u - kp.x, ey = Q.v - kp.y, er = Q.ur - uright[idx];
                    const float e2 = ex * ex + ey * ey + er * er;
                    if (e2 * inv_sigma2[kpLevel] > 7.8) continue;
                } else {
                    const float ex = Q.u - kp.x, ey = Q.v - kp.y;
                    const float e2 = ex * ex + ey * ey;
                    if (e2 * inv_sigma2[kpLevel] > 5.99) continue;
                }
            }
            const int dist = hamming32(dq, desc + 32 * (size_t)idx);
            if (dist < bestDist) { bestDist = dist; bestIdx = idx; }
        }
        if (bestDist <= th_dist) {
            q_idx[iq] = bestIdx;
            q_dist[iq] = bestDist;
            if (fuse) { nmatches++; continue; }   // actions on the map stay with the caller
            has[bestIdx] = 1; obs[bestIdx] = (Q.flags >> 1) & 1;
            kp_final[bestIdx] = iq;
            nmatches++;
            if (check_ori && (variant == ORBO_PROJ_LASTFRAME || variant == ORBO_PROJ_KEYFRAME)) {
                float rot = Q.angle - keys[bestIdx].angle;
                if (rot < 0.0) rot += 360.0f;
                int bin = (int)std::round(rot * factor);
                if (bin == HL) bin = 0;
                rotHist[bin].push_back(iq);
            }
        }
    }
    if (check_ori && (variant == ORBO_PROJ_LASTFRAME || variant == ORBO_PROJ_KEYFRAME)) {
        int sizes[HL];
        for (int i = 0; i < HL; ++i) sizes[i] = (int)rotHist[i].size();
        int ind1, ind2, ind3;
        three_maxima(sizes, HL, ind1, ind2, ind3);
        for (int i = 0; i < HL; i++) {
            if (i == ind1 || i == ind2 || i == ind3) continue;
            for (int iq : rotHist[i]) { kp_final[q_idx[iq]] = -2; q_idx[iq] = -1; nmatches--; }
        }
    }
    return nmatches;
}

// ---- BoW matchers: SearchByBoW x2 (ORBmatcher.cc:160-289, 524-657) and
//      SearchForTriangulation (:659-825 with CheckDistEpipolarLine :140-157) ----
namespace {

struct BowView {   // DBoW2::FeatureVector as CSR
    const uint32_t *ids; const int32_t *off; const int32_t *feat; int nn;
};

// Common nodes in ascending id order (the reference's lower_bound merge join).
template <typename F>
void for_common_nodes(const BowView &A, const BowView &B, F f) {
    int i = 0, j = 0;
    while (i < A.nn && j < B.nn) {
        if (A.ids[i] == B.ids[j]) { f(i, j); ++i; ++j; }
        else if (A.ids[i] < B.ids[j]) { while (i < A.nn && A.ids[i] < B.ids[j]) ++i; }
        else { while (j < B.nn && B.ids[j] < A.ids[i]) ++j; }
    }
}

bool check_dist_epipolar_line(const orbo_keypoint &kp1, const orbo_keypoint &kp2, const float *F12,
                              float sigma2) {
    const float a = kp1.x * F12[0] + kp1.y * F12[3] + F12[6];
    const float b = kp1.x * F12[1] + kp1.y * F12[4] + F12[7];
    const float c = kp1.x * F12[2] + kp1.y * F12[5] + F12[8];
    const float num = a * kp2.x + b * kp2.y + c;
    const float den = a * a + b * b;
    if (den == 0) return false;
    const float dsqr = num * num / den;
    return dsqr < 3.84 * sigma2;
}

}  // namespace

int orbo_search_by_bow(int variant, const orbo_keypoint *ka, const uint8_t *da, const uint8_t *fa, int na,
                       const uint32_t *ida, const int32_t *offa, const int32_t *feata, int nna,
                       const orbo_keypoint *kb, const uint8_t *db, const uint8_t *fb, int nb,
                       const uint32_t *idb, const int32_t *offb, const int32_t *featb, int nnb,
                       float nnratio, int check_ori, const float *tri, int nlevels,
                       int32_t *match_a, int32_t *match_b) {
    const int HL = 30, TH_LOW = 50;
    const float factor = 1.0f / HL;
    std::vector<int> rotHist[HL];
    for (int i = 0; i < na; ++i) match_a[i] = -1;
    for (int i = 0; i < nb; ++i) match_b[i] = -1;
    std::vector<char> matched2(nb, 0);
    int nmatches = 0;
    const BowView A{ida, offa, feata, nna}, B{idb, offb, featb, nnb};
    // triangulation parameters: F12 (row-major 3x3), epipole (ex, ey), then
    // KF2's mvScaleFactors[nlevels] and mvLevelSigma2[nlevels]
    const float *F12 = tri, *scale2 = tri ? tri + 11 : nullptr, *sigma2 = tri ? tri + 11 + nlevels : nullptr;
    const float ex = tri ? tri[9] : 0.f, ey = tri ? tri[10] : 0.f;
    for_common_nodes(A, B, [&](int na_i, int nb_i) {
        for (int p = A.off[na_i]; p < A.off[na_i + 1]; ++p) {
            const int i1 = A.feat[p];
            if (!(fa[i1] & 1)) continue;
            if (variant == ORBO_BOW_TRIANGULATION) {
                const bool bStereo1 = (fa[i1] >> 1) & 1;
                int bestDist = TH_LOW, bestIdx2 = -1;
                for (int q = B.off[nb_i]; q < B.off[nb_i + 1]; ++q) {
                    const int i2 = B.feat[q];
                    if (matched2[i2] || !(fb[i2] & 1)) continue;
                    const bool bStereo2 = (fb[i2] >> 1) & 1;
                    const int dist = hamming32(da + 32 * (size_t)i1, db + 32 * (size_t)i2);
                    if (dist > TH_LOW || dist > bestDist) continue;
                    const orbo_keypoint &kp2 = kb[i2];
                    // an octave outside [0, nlevels) has no table entry (the reference reads past
                    // mvScaleFactors / mvLevelSigma2): both count as 0, as in liborbx, so the pair is rejected
                    const bool lv = kp2.octave >= 0 && kp2.octave < nlevels;
                    if (!bStereo1 && !bStereo2) {
                        const float distex = ex - kp2.x, distey = ey - kp2.y;
                        if (distex * distex + distey * distey < 100 * (lv ? scale2[kp2.octave] : 0.0f)) continue;
                    }
                    if (check_dist_epipolar_line(ka[i1], kp2, F12, lv ? sigma2[kp2.octave] : 0.0f)) { bestIdx2 = i2; bestDist = dist; }
                }
                if (bestIdx2 >= 0) {
                    match_a[i1] = bestIdx2;
                    nmatches++;
                    if (check_ori) {
                        float rot = ka[i1].angle - kb[bestIdx2].angle;
                        if (rot < 0.0) rot += 360.0f;
                        int bin = (int)std::round(rot * factor);
                        if (bin == HL) bin = 0;
                        rotHist[bin].push_back(i1);
                    }
                }
                continue;
            }
            int bestDist1 = 256, bestIdx2 = -1, bestDist2 = 256;
            for (int q = B.off[nb_i]; q < B.off[nb_i + 1]; ++q) {
                const int i2 = B.feat[q];
                if (variant == ORBO_BOW_KF_FRAME) { if (match_b[i2] >= 0) continue; }
                else if (matched2[i2] || !(fb[i2] & 1)) continue;
                const int dist = hamming32(da + 32 * (size_t)i1, db + 32 * (size_t)i2);
                if (dist < bestDist1) { bestDist2 = bestDist1; bestDist1 = dist; bestIdx2 = i2; }
                else if (dist < bestDist2) { bestDist2 = dist; }
            }
            const bool pass = variant == ORBO_BOW_KF_FRAME ? bestDist1 <= TH_LOW : bestDist1 < TH_LOW;
            if (pass && static_cast<float>(bestDist1) < nnratio * static_cast<float>(bestDist2)) {
                match_a[i1] = bestIdx2;
                match_b[bestIdx2] = i1;
                matched2[bestIdx2] = 1;
                if (check_ori) {
                    float rot = ka[i1].angle - kb[bestIdx2].angle;
                    if (rot < 0.0) rot += 360.0f;
                    int bin = (int)std::round(rot * factor);
                    if (bin == HL) bin = 0;
                    rotHist[bin].push_back(i1);
                }
                nmatches++;
            }
        }
    });
    if (check_ori) {
        int sizes[HL];
        for (int i = 0; i < HL; ++i) sizes[i] = (int)rotHist[i].size();
        int ind1, ind2, ind3;
        three_maxima(sizes, HL, ind1, ind2, ind3);
        for (int i = 0; i < HL; i++) {
            if (i == ind1 || i == ind2 || i == ind3) continue;
            for (int i1 : rotHist[i]) {
                if (match_a[i1] >= 0 && variant != ORBO_BOW_TRIANGULATION) match_b[match_a[i1]] = -1;
                match_a[i1] = -1;
                nmatches--;
            }
        }
    }
    return nmatches;
}

// SearchBySim3 (ORBmatcher.cc:1104-1328): two independent best-only window
// searches (INT_MAX start, octave in [pred-1, pred], TH_HIGH) and the
// agreement check.  q1 / q2 carry one row per keyframe map-point slot.
int orbo_search_by_sim3(const orbo_keypoint *k1, const uint8_t *dsc1, int n1, const orbo_keypoint *k2,
                        const uint8_t *dsc2, int n2, float minx1, float maxx1, float miny1, float maxy1,
                        float minx2, float maxx2, float miny2, float maxy2, const orbo_proj_query *q1,
                        const uint8_t *qd1, const orbo_proj_query *q2, const uint8_t *qd2, int th_dist,
                        int32_t *matches12) {
    const FeatureGrid g1(k1, n1, minx1, maxx1, miny1, maxy1), g2(k2, n2, minx2, maxx2, miny2, maxy2);
    auto search = [&](const FeatureGrid &g, const orbo_keypoint *k, const uint8_t *dsc, const orbo_proj_query &Q,
                      const uint8_t *dq) {
        if (!(Q.flags & 1)) return -1;
        int bestDist = INT_MAX, bestIdx = -1;
        for (int idx : g.area(k, Q.u, Q.v, Q.radius, -1, -1)) {
            if (k[idx].octave < Q.min_level || k[idx].octave > Q.max_level) continue;
            const int dist = hamming32(dq, dsc + 32 * (size_t)idx);
            if (dist < bestDist) { bestDist = dist; bestIdx = idx; }
        }
        return bestDist <= th_dist ? bestIdx : -1;
    };
    std::vector<int> m1(n1, -1), m2(n2, -1);
    for (int i1 = 0; i1 < n1; ++i1) m1[i1] = search(g2, k2, dsc2, q1[i1], qd1 + 32 * (size_t)i1);
    for (int i2 = 0; i2 < n2; ++i2) m2[i2] = search(g1, k1, dsc1, q2[i2], qd2 + 32 * (size_t)i2);
    int nFound = 0;
    for (int i1 = 0; i1 < n1; ++i1) {
        matches12[i1] = -1;
        const int idx2 = m1[i1];
        if (idx2 >= 0 && m2[idx2] == i1) { matches12[i1] = idx2; nFound++; }
    }
    return nFound;
}

// ---------------------------------------------------------------------------
// DBoW2 vocabulary transform (TemplatedVocabulary.h:1140-1272).
struct OrboVocab {
    std::vector<std::vector<int>> children;
    std::vector<uint32_t> word_id;
    int nwords = 0;
};

// The loaders' tree: children in file order, word ids in leaf-flag order.
void *orbo_vocab_prepare(int n_nodes, const int32_t *parent, const uint8_t *is_leaf) {
    OrboVocab *t = new OrboVocab;
    t->children.resize(n_nodes);
    t->word_id.assign(n_nodes, 0);   // Node(): word_id(0)
    for (int i = 1; i < n_nodes; ++i) {
        t->children[parent[i]].push_back(i);
        if (is_leaf[i]) t->word_id[i] = (uint32_t)t->nwords++;
    }
    return t;
}

void orbo_vocab_release(void *t) { delete static_cast<OrboVocab *>(t); }

int orbo_vocab_transform(int L, int scoring, int weighting, int n_nodes, const int32_t *parent,
                         const uint8_t *is_leaf, const uint8_t *desc, const double *weight,
                         const uint8_t *features, int n, int levelsup,
                         uint32_t *bow_words, double *bow_values, int *n_bow,
                         uint32_t *fv_nodes, int32_t *fv_offsets, int32_t *fv_features, int *n_fv,
                         uint32_t *f_word, double *f_weight, uint32_t *f_node) {
    OrboVocab *t = static_cast<OrboVocab *>(orbo_vocab_prepare(n_nodes, parent, is_leaf));
    const int r = orbo_vocab_transform_prepared(t, L, scoring, weighting, desc, weight, features, n, levelsup,
                                                bow_words, bow_values, n_bow, fv_nodes, fv_offsets, fv_features,
                                                n_fv, f_word, f_weight, f_node);
    delete t;
    return r;
}

int orbo_vocab_transform_prepared(void *tree, int L, int scoring, int weighting, const uint8_t *desc,
                                  const double *weight, const uint8_t *features, int n, int levelsup,
                                  uint32_t *bow_words, double *bow_values, int *n_bow,
                                  uint32_t *fv_nodes, int32_t *fv_offsets, int32_t *fv_features, int *n_fv,
                                  uint32_t *f_word, double *f_weight, uint32_t *f_node) {
    const OrboVocab &T = *static_cast<const OrboVocab *>(tree);
    const std::vector<std::vector<int>> &children = T.children;
    const std::vector<uint32_t> &word_id = T.word_id;
    const int nwords = T.nwords;
    *n_bow = 0;
    *n_fv = 0;
    if (fv_offsets) fv_offsets[0] = 0;
    if (nwords == 0) return 0;   // empty()
    // normalisation of the scoring object (ScoringObject.h:74-89)
    const bool must = scoring != 5;              // DOT_PRODUCT does not normalise
    const bool l2 = scoring == 1;                // L2_NORM; the others are L1
    std::map<uint32_t, double> bow;
    std::map<uint32_t, std::vector<int>> fv;
    const int nid_level = L - levelsup;
    for (int f = 0; f < n; ++f) {
        const uint8_t *fd = features + 32 * (size_t)f;
        uint32_t nid = 0;   // (set at nid_level; a shallower leaf keeps the leaf, see header)
        int final_id = 0, level = 0;
        bool nid_set = nid_level <= 0;
        do {
            ++level;
            const std::vector<int> &nodes = children[final_id];
            final_id = nodes[0];
            double best_d = hamming32(fd, desc + 32 * (size_t)final_id);
            for (size_t c = 1; c < nodes.size(); ++c) {
                const double d = hamming32(fd, desc + 32 * (size_t)nodes[c]);
                if (d < best_d) { best_d = d; final_id = nodes[c]; }
            }
            if (level == nid_level) { nid = (uint32_t)final_id; nid_set = true; }
        } while (!children[final_id].empty());
        if (!nid_set) nid = (uint32_t)final_id;
        const uint32_t wid = word_id[final_id];
        const double w = weight[final_id];
        if (f_word) f_word[f] = wid;
        if (f_weight) f_weight[f] = w;
        if (f_node) f_node[f] = nid;
        if (w > 0) {
            if (weighting == 0 || weighting == 1) {   // TF_IDF, TF: addWeight
                auto it = bow.find(wid);
                if (it == bow.end()) bow.emplace(wid, w); else it->second += w;
            } else {                                  // IDF, BINARY: addIfNotExist
                bow.emplace(wid, w);
            }
            fv[nid].push_back(f);
        }
    }
    if ((weighting == 0 || weighting == 1) && !bow.empty() && !must) {
        const double nd = (double)bow.size();
        for (auto &kv : bow) kv.second /= nd;
    }
    if (must) {
        double norm = 0.0;
        if (!l2) {
            for (auto &kv : bow) norm += std::fabs(kv.second);
        } else {
            for (auto &kv : bow) norm += kv.second * kv.second;
            norm = std::sqrt(norm);
        }
        if (norm > 0.0)
            for (auto &kv : bow) kv.second /= norm;
    }
    int i = 0;
    for (auto &kv : bow) { bow_words[i] = kv.first; bow_values[i] = kv.second; ++i; }
    *n_bow = i;
    int j = 0, t = 0;
    for (auto &kv : fv) {
        fv_nodes[j] = kv.first;
        for (int x : kv.second) fv_features[t++] = x;
        fv_offsets[++j] = t;
    }
    *n_fv = j;
    return nwords;
}

// ---------------------------------------------------------------------------
// MapPoint::ComputeDistinctiveDescriptors (MapPoint.cc:288-361).
void orbo_distinctive_descriptors(const uint8_t *desc, const int32_t *offsets, int np, int32_t *best) {
    for (int p = 0; p < np; ++p) {
        const int o = offsets[p];
        const size_t N = (size_t)(offsets[p + 1] - o);
        if (N == 0) { best[p] = -1; continue; }
        std::vector<float> D(N * N);
        for (size_t i = 0; i < N; i++) {
            D[i * N + i] = 0;
            for (size_t j = i + 1; j < N; j++) {
                const int distij = hamming32(desc + 32 * (size_t)(o + i), desc + 32 * (size_t)(o + j));
                D[i * N + j] = (float)distij;
                D[j * N + i] = (float)distij;
            }
        }
        int BestMedian = INT_MAX, BestIdx = 0;
        for (size_t i = 0; i < N; i++) {
            std::vector<int> v(D.begin() + i * N, D.begin() + (i + 1) * N);
            std::sort(v.begin(), v.end());
            const int median = v[(size_t)(0.5 * (N - 1))];
            if (median < BestMedian) { BestMedian = median; BestIdx = (int)i; }
        }
        best[p] = BestIdx;
    }
}

// cv::undistortPoints (OpenCV 3.2 cvUndistortPoints, modules/imgproc/src/
// undistort.cpp) with R = I and P = K, as Frame::UndistortKeyPoints calls it.
void orbo_undistort_points(const float *xy_in, int n, const float *K, const float *dist, int ncoef, float *xy_out) {
    if (dist[0] == 0.0f) {   // Frame.cc:441: mvKeysUn = mvKeys
        std::memcpy(xy_out, xy_in, sizeof(float) * 2 * (size_t)n);
        return;
    }
    double k[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int i = 0; i < ncoef && i < 8; ++i) k[i] = dist[i];
    const double fx = K[0], fy = K[4], cx = K[2], cy = K[5];
    const double ifx = 1. / fx, ify = 1. / fy;
    // RR = P * I = K (cvMatMul of exact 0/1 entries)
    const double RR[3][3] = {{K[0], K[1], K[2]}, {K[3], K[4], K[5]}, {K[6], K[7], K[8]}};
    for (int i = 0; i < n; i++) {
        double x = xy_in[2 * i], y = xy_in[2 * i + 1], x0, y0;
        x0 = x = (x - cx) * ifx;
        y0 = y = (y - cy) * ify;
        for (int j = 0; j < 5; j++) {
            const double r2 = x * x + y * y;
            const double icdist = (1 + ((k[7] * r2 + k[6]) * r2 + k[5]) * r2) / (1 + ((k[4] * r2 + k[1]) * r2 + k[0]) * r2);
            const double deltaX = 2 * k[2] * x * y + k[3] * (r2 + 2 * x * x);
            const double deltaY = k[2] * (r2 + 2 * y * y) + 2 * k[3] * x * y;
            x = (x0 - deltaX) * icdist;
            y = (y0 - deltaY) * icdist;
        }
        const double xx = RR[0][0] * x + RR[0][1] * y + RR[0][2];
        const double yy = RR[1][0] * x + RR[1][1] * y + RR[1][2];
        const double ww = 1. / (RR[2][0] * x + RR[2][1] * y + RR[2][2]);
        xy_out[2 * i] = (float)(xx * ww);
        xy_out[2 * i + 1] = (float)(yy * ww);
    }
}

// cvtColor *2GRAY for 8U (OpenCV 3.2 RGB2Gray<uchar>: 14-bit fixed point).
void orbo_cvt_gray(const uint8_t *src, int w, int h, size_t spitch, int channels, int rgb, uint8_t *dst,
                   size_t dpitch) {
    const int R2Y = 4899, G2Y = 9617, B2Y = 1868, shift = 14;
    const int bidx = rgb ? 2 : 0;
    for (int y = 0; y < h; ++y)
        for (int x = 0; x < w; ++x) {
            const uint8_t *s = src + y * spitch + (size_t)x * channels;
            dst[y * dpitch + x] =
                (uint8_t)((s[bidx] * B2Y + s[1] * G2Y + s[bidx ^ 2] * R2Y + (1 << (shift - 1))) >> shift);
        }
}

// Mat::convertTo(CV_32F, scale) from 16U.
void orbo_depth_to_float(const uint16_t *src, int w, int h, size_t spitch, float scale, float *dst, size_t dpitch) {
    for (int y = 0; y < h; ++y) {
        const uint16_t *s = reinterpret_cast<const uint16_t *>(reinterpret_cast<const uint8_t *>(src) + y * spitch);
        float *d = reinterpret_cast<float *>(reinterpret_cast<uint8_t *>(dst) + y * dpitch);
        for (int x = 0; x < w; ++x) d[x] = (float)s[x] * scale;
    }
}

// ---------------------------------------------------------------------------
// KeyFrameDatabase (KeyFrameDatabase.cc:31-236) over named keyframes.
namespace {
struct OrboKF {
    uint64_t id;
    std::vector<uint32_t> words;
    std::vector<double> values;
    uint64_t mnLoopQuery = 0, mnRelocQuery = 0;   // KeyFrame.cc:41
    int mnLoopWords = 0, mnRelocWords = 0;
    float mLoopScore = 0, mRelocScore = 0;        // uninitialised in the reference
};
struct OrboKFDB {
    std::vector<std::list<OrboKF *>> inv;
    std::unordered_map<uint64_t, OrboKF *> kfs;
    std::vector<OrboKF *> owned;
};

// L1Scoring::score (ScoringObject.cpp:23-66): merge with lower_bound jumps;
// only common words add, in ascending word order.
double l1_score(const uint32_t *w1, const double *v1, int n1, const uint32_t *w2, const double *v2, int n2) {
    int i = 0, j = 0;
    double score = 0;
    while (i < n1 && j < n2) {
        const double vi = v1[i], wi = v2[j];
        if (w1[i] == w2[j]) {
            score += std::fabs(vi - wi) - std::fabs(vi) - std::fabs(wi);
            ++i;
            ++j;
        } else if (w1[i] < w2[j]) {
            i = (int)(std::lower_bound(w1, w1 + n1, w2[j]) - w1);
        } else {
            j = (int)(std::lower_bound(w2, w2 + n2, w1[i]) - w2);
        }
    }
    return -score / 2.0;
}
}  // namespace

double orbo_bow_score_l1(const uint32_t *w1, const double *v1, int n1, const uint32_t *w2, const double *v2, int n2) {
    return l1_score(w1, v1, n1, w2, v2, n2);
}

void *orbo_kfdb_create(int n_words) {
    OrboKFDB *db = new OrboKFDB;
    db->inv.resize(n_words);
    return db;
}

void orbo_kfdb_destroy(void *p) {
    OrboKFDB *db = static_cast<OrboKFDB *>(p);
    for (OrboKF *k : db->owned) delete k;
    delete db;
}

void orbo_kfdb_add(void *p, uint64_t kf_id, const uint32_t *words, const double *values, int n) {
    OrboKFDB *db = static_cast<OrboKFDB *>(p);
    OrboKF *k;
    auto it = db->kfs.find(kf_id);
    if (it != db->kfs.end()) {
        k = it->second;
    } else {
        k = new OrboKF;
        k->id = kf_id;
        k->words.assign(words, words + n);
        k->values.assign(values, values + n);
        db->kfs[kf_id] = k;
        db->owned.push_back(k);
    }
    for (int i = 0; i < n; ++i) db->inv[words[i]].push_back(k);
}

void orbo_kfdb_erase(void *p, uint64_t kf_id) {
    OrboKFDB *db = static_cast<OrboKFDB *>(p);
    auto it = db->kfs.find(kf_id);
    if (it == db->kfs.end()) return;
    OrboKF *k = it->second;
    for (uint32_t w : k->words) {
        std::list<OrboKF *> &l = db->inv[w];
        for (auto lit = l.begin(); lit != l.end(); ++lit)
            if (*lit == k) { l.erase(lit); break; }
    }
}

void orbo_kfdb_clear(void *p) {
    OrboKFDB *db = static_cast<OrboKFDB *>(p);
    const size_t nw = db->inv.size();
    db->inv.clear();
    db->inv.resize(nw);
}

int orbo_kfdb_detect(void *p, int reloc, uint64_t qid, const uint32_t *words, const double *values, int n,
                     const uint64_t *connected, int n_connected, float minScore, orbo_covis_fn covis, void *ctx,
                     uint64_t *out, int cap) {
    OrboKFDB *db = static_cast<OrboKFDB *>(p);
    std::set<uint64_t> conn(connected, connected + (reloc ? 0 : n_connected));
    std::list<OrboKF *> sharing;
    for (int i = 0; i < n; ++i) {
        for (OrboKF *k : db->inv[words[i]]) {
            if (!reloc) {
                if (k->mnLoopQuery != qid) {
                    k->mnLoopWords = 0;
                    if (!conn.count(k->id)) {
                        k->mnLoopQuery = qid;
                        sharing.push_back(k);
                    }
                }
                k->mnLoopWords++;
            } else {
                if (k->mnRelocQuery != qid) {
                    k->mnRelocWords = 0;
                    k->mnRelocQuery = qid;
                    sharing.push_back(k);
                }
                k->mnRelocWords++;
            }
        }
    }
    if (sharing.empty()) return 0;
    int maxCommonWords = 0;
    for (OrboKF *k : sharing) maxCommonWords = std::max(maxCommonWords, reloc ? k->mnRelocWords : k->mnLoopWords);
    const int minCommonWords = maxCommonWords * 0.8f;
    std::list<std::pair<float, OrboKF *>> scored;
    for (OrboKF *k : sharing) {
        if ((reloc ? k->mnRelocWords : k->mnLoopWords) > minCommonWords) {
            const float si = (float)l1_score(words, values, n, k->words.data(), k->values.data(), (int)k->words.size());
            if (reloc) {
                k->mRelocScore = si;
                scored.push_back(std::make_pair(si, k));
            } else {
                k->mLoopScore = si;
                if (si >= minScore) scored.push_back(std::make_pair(si, k));
            }
        }
    }
    if (scored.empty()) return 0;
    std::list<std::pair<float, OrboKF *>> acc;
    float bestAccScore = reloc ? 0 : minScore;
    uint64_t neigh[64];
    for (auto &sm : scored) {
        OrboKF *ki = sm.second;
        const int nn = covis(ctx, ki->id, neigh, 10);
        float bestScore = sm.first, accScore = sm.first;
        OrboKF *best = ki;
        for (int t = 0; t < nn; ++t) {
            auto it = db->kfs.find(neigh[t]);
            if (it == db->kfs.end()) continue;   // (a neighbour never added holds no query state)
            OrboKF *k2 = it->second;
            if (!reloc) {
                if (k2->mnLoopQuery == qid && k2->mnLoopWords > minCommonWords) {
                    accScore += k2->mLoopScore;
                    if (k2->mLoopScore > bestScore) { best = k2; bestScore = k2->mLoopScore; }
                }
            } else {
                if (k2->mnRelocQuery != qid) continue;
                accScore += k2->mRelocScore;
                if (k2->mRelocScore > bestScore) { best = k2; bestScore = k2->mRelocScore; }
            }
        }
        acc.push_back(std::make_pair(accScore, best));
        if (accScore > bestAccScore) bestAccScore = accScore;
    }
    const float minScoreToRetain = 0.75f * bestAccScore;
    std::set<OrboKF *> added;
    int m = 0;
    for (auto &a : acc) {
        if (a.first > minScoreToRetain && !added.count(a.second)) {
            if (m < cap) out[m] = a.second->id;
            ++m;
            added.insert(a.second);
        }
    }
    return m;
}

// ---------------------------------------------------------------------------
// Local bundle adjustment (Optimizer.cc:517-900 over g2o).
namespace {
struct BQ { double q[4], t[3]; int f; };   // SE3Quat (x y z w), free index or -1

void bq_rot(const double *q, const double *v, double *o) {   // Eigen _transformVector
    double uv[3] = {q[1] * v[2] - q[2] * v[1], q[2] * v[0] - q[0] * v[2], q[0] * v[1] - q[1] * v[0]};
    for (int i = 0; i < 3; ++i) uv[i] = uv[i] + uv[i];
    const double c[3] = {q[1] * uv[2] - q[2] * uv[1], q[2] * uv[0] - q[0] * uv[2], q[0] * uv[1] - q[1] * uv[0]};
    for (int i = 0; i < 3; ++i) o[i] = v[i] + q[3] * uv[i] + c[i];
}
void bq_R(const double *q, double *R) {   // toRotationMatrix
    const double tx = 2 * q[0], ty = 2 * q[1], tz = 2 * q[2];
    const double twx = tx * q[3], twy = ty * q[3], twz = tz * q[3];
    const double txx = tx * q[0], txy = ty * q[0], txz = tz * q[0];
    const double tyy = ty * q[1], tyz = tz * q[1], tzz = tz * q[2];
    const double r[9] = {1 - (tyy + tzz), txy - twz, txz + twy, txy + twz, 1 - (txx + tzz), tyz - twx,
                         txz - twy, tyz + twx, 1 - (txx + tyy)};
    std::memcpy(R, r, sizeof(r));
}
void bq_fromR(const double *m, double *q) {   // Quaternion(Matrix3d)
    const double tr = m[0] + m[4] + m[8];
    if (tr > 0) {
        double t = std::sqrt(tr + 1.0);
        q[3] = 0.5 * t;
        t = 0.5 / t;
        q[0] = (m[7] - m[5]) * t;
        q[1] = (m[2] - m[6]) * t;
        q[2] = (m[3] - m[1]) * t;
    } else {
        int i = 0;
        if (m[4] > m[0]) i = 1;
        if (m[8] > m[3 * i + i]) i = 2;
        const int j = (i + 1) % 3, k = (j + 1) % 3;
        double t = std::sqrt(m[3 * i + i] - m[3 * j + j] - m[3 * k + k] + 1.0);
        q[i] = 0.5 * t;
        t = 0.5 / t;
        q[3] = (m[3 * k + j] - m[3 * j + k]) * t;
        q[j] = (m[3 * j + i] + m[3 * i + j]) * t;
        q[k] = (m[3 * k + i] + m[3 * i + k]) * t;
    }
}
void bq_norm(double *q) {   // normalizeRotation
    if (q[3] < 0)
        for (int i = 0; i < 4; ++i) q[i] *= -1;
    const double n = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    for (int i = 0; i < 4; ++i) q[i] = q[i] / n;
}
void bq_mul(const double *a, const double *b, double *o) {
    o[3] = a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2];
    o[0] = a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1];
    o[1] = a[3] * b[1] + a[1] * b[3] + a[2] * b[0] - a[0] * b[2];
    o[2] = a[3] * b[2] + a[2] * b[3] + a[0] * b[1] - a[1] * b[0];
}

struct OBA {
    int ncam, npt, ne, nf;
    std::vector<BQ> T;
    std::vector<double> X;
    const orbo_ba_edge *E;
    std::vector<double> delta, err, chi2, rho0, rho1;
    std::vector<uint8_t> act, front;
    std::vector<std::vector<int>> pe;     // edges per point, by camera
    std::vector<std::vector<int>> ce;     // edges per free camera, edge order
    // system
    std::vector<double> Hpp, bp, Hll, bl, hpp_e, hll_e, hpl_e, bp_e, bl_e, x;
    bool robust = true;

    void proj(int e, double *p) const {
        const BQ &t = T[E[e].cam];
        bq_rot(t.q, &X[3 * (size_t)E[e].point], p);
        for (int i = 0; i < 3; ++i) p[i] = p[i] + t.t[i];
    }
    void fronts() {   // isDepthPositive() at the current estimate, errors untouched
        for (int e = 0; e < ne; ++e) {
            double p[3];
            proj(e, p);
            front[e] = p[2] > 0.0;
        }
    }
    double errors() {
        double s = 0;
        for (int e = 0; e < ne; ++e) {
            double p[3];
            proj(e, p);
            front[e] = p[2] > 0.0;
            if (!act[e]) continue;
            const orbo_ba_edge &d = E[e];
            const bool st = d.ur >= 0;
            double r[3];
            if (!st) {
                const double u = p[0] / p[2], v = p[1] / p[2];
                r[0] = (double)d.u - (u * (double)d.fx + (double)d.cx);
                r[1] = (double)d.v - (v * (double)d.fy + (double)d.cy);
                r[2] = 0;
            } else {
                const double invz = (double)(float)(1.0 / p[2]);
                const double r0 = p[0] * invz * (double)d.fx + (double)d.cx;
                const double r1 = p[1] * invz * (double)d.fy + (double)d.cy;
                r[0] = (double)d.u - r0;
                r[1] = (double)d.v - r1;
                r[2] = (double)d.ur - (r0 - (double)d.bf * invz);
            }
            const double om = d.inv_sigma2;
            double c = 0;
            for (int k = 0; k < (st ? 3 : 2); ++k) c = c + r[k] * (om * r[k]);
            double a0 = c, a1 = 1.0;
            if (robust) {
                const double dsqr = delta[e] * delta[e];
                if (!(c <= dsqr)) {
                    const double sq = std::sqrt(c);
                    a0 = 2 * sq * delta[e] - dsqr;
                    a1 = delta[e] / sq;
                }
            }
            for (int k = 0; k < 3; ++k) err[3 * (size_t)e + k] = r[k];
            chi2[e] = c;
            rho0[e] = a0;
            rho1[e] = a1;
            s += a0;
        }
        return s;
    }
    void linearize(int e) {
        const orbo_ba_edge &d = E[e];
        const bool st = d.ur >= 0;
        const double fx = d.fx, fy = d.fy, bf = d.bf;
        double p[3];
        proj(e, p);
        const double x = p[0], y = p[1], z = p[2], z_2 = z * z;
        double R[9];
        bq_R(T[d.cam].q, R);
        double A[3][3], B[3][6];
        if (!st) {
            const double tmp[2][3] = {{fx, 0, -x / z * fx}, {0, fy, -y / z * fy}};
            const double s = -1. / z;
            for (int r = 0; r < 2; ++r)
                for (int c = 0; c < 3; ++c) {
                    double acc = 0;
                    for (int k = 0; k < 3; ++k) acc = acc + (s * tmp[r][k]) * R[3 * k + c];
                    A[r][c] = acc;
                }
        } else {
            for (int c = 0; c < 3; ++c) {
                A[0][c] = -fx * R[c] / z + fx * x * R[6 + c] / z_2;
                A[1][c] = -fy * R[3 + c] / z + fy * y * R[6 + c] / z_2;
                A[2][c] = A[0][c] - bf * R[6 + c] / z_2;
            }
        }
        B[0][0] = x * y / z_2 * fx; B[0][1] = -(1 + (x * x / z_2)) * fx; B[0][2] = y / z * fx;
        B[0][3] = -1. / z * fx; B[0][4] = 0; B[0][5] = x / z_2 * fx;
        B[1][0] = (1 + y * y / z_2) * fy; B[1][1] = -x * y / z_2 * fy; B[1][2] = -x / z * fy;
        B[1][3] = 0; B[1][4] = -1. / z * fy; B[1][5] = y / z_2 * fy;
        if (st) {
            B[2][0] = B[0][0] - bf * y / z_2; B[2][1] = B[0][1] + bf * x / z_2; B[2][2] = B[0][2];
            B[2][3] = B[0][3]; B[2][4] = 0; B[2][5] = B[0][5] - bf / z_2;
        }
        const int D = st ? 3 : 2;
        const double w = rho1[e] * (double)d.inv_sigma2;
        double omr[3];
        for (int k = 0; k < D; ++k) omr[k] = -((double)d.inv_sigma2 * err[3 * (size_t)e + k]) * rho1[e];
        const bool pf = T[d.cam].f >= 0;
        for (int a = 0; a < 3; ++a)
            for (int b = 0; b < 3; ++b) {
                double acc = 0;
                for (int k = 0; k < D; ++k) acc = acc + (A[k][a] * w) * A[k][b];
                hll_e[9 * (size_t)e + 3 * a + b] = acc;
            }
        for (int a = 0; a < 6; ++a) {
            for (int b = 0; b < 6; ++b) {
                double acc = 0;
                if (pf)
                    for (int k = 0; k < D; ++k) acc = acc + (B[k][a] * w) * B[k][b];
                hpp_e[36 * (size_t)e + 6 * a + b] = acc;
            }
            for (int c = 0; c < 3; ++c) {
                double acc = 0;
                if (pf)
                    for (int k = 0; k < D; ++k) acc = acc + (A[k][c] * w) * B[k][a];
                hpl_e[18 * (size_t)e + 3 * a + c] = acc;
            }
            double acc = 0;
            if (pf)
                for (int k = 0; k < D; ++k) acc = acc + B[k][a] * omr[k];
            bp_e[6 * (size_t)e + a] = acc;
        }
        for (int c = 0; c < 3; ++c) {
            double acc = 0;
            for (int k = 0; k < D; ++k) acc = acc + A[k][c] * omr[k];
            bl_e[3 * (size_t)e + c] = acc;
        }
    }
    void build() {
        for (int e = 0; e < ne; ++e)
            if (act[e]) linearize(e);
        Hpp.assign(36 * (size_t)nf, 0); bp.assign(6 * (size_t)nf, 0);
        Hll.assign(9 * (size_t)npt, 0); bl.assign(3 * (size_t)npt, 0);
        for (int f = 0; f < nf; ++f)
            for (int e : ce[f]) {
                if (!act[e]) continue;
                for (int k = 0; k < 36; ++k) Hpp[36 * (size_t)f + k] = Hpp[36 * (size_t)f + k] + hpp_e[36 * (size_t)e + k];
                for (int k = 0; k < 6; ++k) bp[6 * (size_t)f + k] = bp[6 * (size_t)f + k] + bp_e[6 * (size_t)e + k];
            }
        for (int p = 0; p < npt; ++p)
            for (int e : pe[p]) {
                if (!act[e]) continue;
                for (int k = 0; k < 9; ++k) Hll[9 * (size_t)p + k] = Hll[9 * (size_t)p + k] + hll_e[9 * (size_t)e + k];
                for (int k = 0; k < 3; ++k) bl[3 * (size_t)p + k] = bl[3 * (size_t)p + k] + bl_e[3 * (size_t)e + k];
            }
    }
    double max_diag() const {
        double m = 0.;
        for (int f = 0; f < nf; ++f)
            for (int j = 0; j < 6; ++j) m = std::max(std::fabs(Hpp[36 * (size_t)f + 7 * j]), m);
        for (int p = 0; p < npt; ++p)
            for (int j = 0; j < 3; ++j) m = std::max(std::fabs(Hll[9 * (size_t)p + 4 * j]), m);
        return m;
    }
    static double cof(const double *m, int i, int j) {
        const int i1 = (i + 1) % 3, i2 = (i + 2) % 3, j1 = (j + 1) % 3, j2 = (j + 2) % 3;
        return m[3 * i1 + j1] * m[3 * i2 + j2] - m[3 * i1 + j2] * m[3 * i2 + j1];
    }
    bool usable(int e) const { return act[e] && T[E[e].cam].f >= 0; }
    bool solve(double lambda) {
        const int n = 6 * nf;
        std::vector<double> S((size_t)n * n, 0.0), bs(n), dinv(9 * (size_t)npt), bdinv(18 * (size_t)ne),
            bdb(6 * (size_t)ne);
        for (int p = 0; p < npt; ++p) {
            double m[9];
            for (int k = 0; k < 9; ++k) m[k] = Hll[9 * (size_t)p + k];
            for (int k = 0; k < 3; ++k) m[4 * k] = m[4 * k] + lambda;
            const double c0 = cof(m, 0, 0), c1 = cof(m, 1, 0), c2 = cof(m, 2, 0);
            const double det = c0 * m[0] + c1 * m[3] + c2 * m[6];
            const double invdet = 1.0 / det;
            double *D = &dinv[9 * (size_t)p];
            D[0] = c0 * invdet; D[1] = c1 * invdet; D[2] = c2 * invdet;
            D[3] = cof(m, 0, 1) * invdet; D[4] = cof(m, 1, 1) * invdet; D[5] = cof(m, 2, 1) * invdet;
            D[6] = cof(m, 0, 2) * invdet; D[7] = cof(m, 1, 2) * invdet; D[8] = cof(m, 2, 2) * invdet;
            double db[3];
            for (int r = 0; r < 3; ++r) {
                double acc = 0;
                for (int c = 0; c < 3; ++c) acc = acc + D[3 * r + c] * bl[3 * (size_t)p + c];
                db[r] = acc;
            }
            for (int e : pe[p]) {
                if (!usable(e)) continue;
                const double *Bm = &hpl_e[18 * (size_t)e];
                for (int r = 0; r < 6; ++r) {
                    for (int c = 0; c < 3; ++c) {
                        double acc = 0;
                        for (int k = 0; k < 3; ++k) acc = acc + Bm[3 * r + k] * D[3 * k + c];
                        bdinv[18 * (size_t)e + 3 * r + c] = acc;
                    }
                    double acc = 0;
                    for (int k = 0; k < 3; ++k) acc = acc + Bm[3 * r + k] * db[k];
                    bdb[6 * (size_t)e + r] = acc;
                }
            }
        }
        // camera lists of usable edges in ascending point order
        std::vector<std::vector<int>> cl(nf);
        for (int p = 0; p < npt; ++p)
            for (int e : pe[p])
                if (usable(e)) cl[T[E[e].cam].f].push_back(e);
        for (int i1 = 0; i1 < nf; ++i1)
            for (int i2 = i1; i2 < nf; ++i2)
                for (int r = 0; r < 6; ++r)
                    for (int c = 0; c < 6; ++c) {
                        double acc = 0;
                        if (i1 == i2) {
                            acc = Hpp[36 * (size_t)i1 + 6 * r + c];
                            if (r == c) acc = acc + lambda;
                        }
                        size_t a = 0, b = 0;
                        while (a < cl[i1].size() && b < cl[i2].size()) {
                            const int pa = E[cl[i1][a]].point, pb = E[cl[i2][b]].point;
                            if (pa < pb) { ++a; continue; }
                            if (pb < pa) { ++b; continue; }
                            // a camera that observes the point more than once adds its
                            // edges into one Hpl block in g2o: every edge of i1 at this
                            // point meets every edge of i2 at it
                            size_t a2 = a, b2 = b;
                            while (a2 < cl[i1].size() && E[cl[i1][a2]].point == pa) ++a2;
                            while (b2 < cl[i2].size() && E[cl[i2][b2]].point == pa) ++b2;
                            for (size_t ia = a; ia < a2; ++ia)
                                for (size_t ib = b; ib < b2; ++ib) {
                                    double s = 0;
                                    for (int k = 0; k < 3; ++k)
                                        s = s + bdinv[18 * (size_t)cl[i1][ia] + 3 * r + k] *
                                                    hpl_e[18 * (size_t)cl[i2][ib] + 3 * c + k];
                                    acc = acc - s;
                                }
                            a = a2;
                            b = b2;
                        }
                        S[(size_t)(6 * i1 + r) * n + 6 * i2 + c] = acc;
                        S[(size_t)(6 * i2 + c) * n + 6 * i1 + r] = acc;
                    }
        for (int i = 0; i < n; ++i) {
            double coef = 0;
            for (int e : cl[i / 6]) coef = coef + bdb[6 * (size_t)e + i % 6];
            bs[i] = bp[i] - coef;
        }
        x.assign(n + 3 * (size_t)npt, 0.0);
        for (int j = 0; j < n; ++j) {   // dense Cholesky, column by column
            double d = S[(size_t)j * n + j];
            for (int k = 0; k < j; ++k) d = d - S[(size_t)j * n + k] * S[(size_t)j * n + k];
            if (!(d > 0)) return false;
            const double dg = std::sqrt(d);
            S[(size_t)j * n + j] = dg;
            for (int i = j + 1; i < n; ++i) {
                double s2 = S[(size_t)i * n + j];
                for (int k = 0; k < j; ++k) s2 = s2 - S[(size_t)i * n + k] * S[(size_t)j * n + k];
                S[(size_t)i * n + j] = s2 / dg;
            }
        }
        for (int i = 0; i < n; ++i) {
            double s2 = bs[i];
            for (int k = 0; k < i; ++k) s2 = s2 - S[(size_t)i * n + k] * x[k];
            x[i] = s2 / S[(size_t)i * n + i];
        }
        for (int i = n - 1; i >= 0; --i) {
            double s2 = x[i];
            for (int k = n - 1; k > i; --k) s2 = s2 - S[(size_t)k * n + i] * x[k];
            x[i] = s2 / S[(size_t)i * n + i];
        }
        for (int p = 0; p < npt; ++p) {
            double c3[3];
            for (int k = 0; k < 3; ++k) c3[k] = bl[3 * (size_t)p + k];
            for (int e : pe[p]) {
                if (!usable(e)) continue;
                const int f = T[E[e].cam].f;
                const double *Bm = &hpl_e[18 * (size_t)e];
                for (int c = 0; c < 3; ++c) {
                    double s2 = 0;
                    for (int r = 0; r < 6; ++r) s2 = s2 + Bm[3 * r + c] * -x[6 * f + r];
                    c3[c] = c3[c] + s2;
                }
            }
            const double *D = &dinv[9 * (size_t)p];
            for (int r = 0; r < 3; ++r) {
                double acc = 0;
                for (int c = 0; c < 3; ++c) acc = acc + D[3 * r + c] * c3[c];
                x[n + 3 * (size_t)p + r] = acc;
            }
        }
        return true;
    }
    double scale(double lambda) const {
        const int n = 6 * nf;
        double s2 = 0.;
        for (int j = 0; j < n; ++j) s2 += x[j] * (lambda * x[j] + bp[j]);
        for (int j = 0; j < 3 * npt; ++j) s2 += x[n + j] * (lambda * x[n + j] + bl[j]);
        return s2;
    }
    void update() {
        const int n = 6 * nf;
        for (int c = 0; c < ncam; ++c) {
            BQ &t = T[c];
            if (t.f < 0) continue;
            const double *u = &x[6 * (size_t)t.f];
            const double w[3] = {u[0], u[1], u[2]}, ups[3] = {u[3], u[4], u[5]};
            const double theta = std::sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
            const double Om[9] = {0, -w[2], w[1], w[2], 0, -w[0], -w[1], w[0], 0};
            double O2[9], R[9], V[9];
            for (int r = 0; r < 3; ++r)
                for (int cc = 0; cc < 3; ++cc) {
                    double acc = 0;
                    for (int k = 0; k < 3; ++k) acc = acc + Om[3 * r + k] * Om[3 * k + cc];
                    O2[3 * r + cc] = acc;
                }
            if (theta < 0.00001) {
                for (int k = 0; k < 9; ++k) R[k] = ((k % 4 == 0) ? 1.0 : 0.0) + Om[k] + O2[k];
                for (int k = 0; k < 9; ++k) V[k] = R[k];
            } else {
                const double a = std::sin(theta) / theta, b = (1 - std::cos(theta)) / (theta * theta);
                const double cc = (theta - std::sin(theta)) / std::pow(theta, 3);
                for (int k = 0; k < 9; ++k) {
                    R[k] = ((k % 4 == 0) ? 1.0 : 0.0) + a * Om[k] + b * O2[k];
                    V[k] = ((k % 4 == 0) ? 1.0 : 0.0) + b * Om[k] + cc * O2[k];
                }
            }
            double qe[4], te[3], rt[3], qn[4];
            bq_fromR(R, qe);
            for (int r = 0; r < 3; ++r) te[r] = V[3 * r] * ups[0] + V[3 * r + 1] * ups[1] + V[3 * r + 2] * ups[2];
            bq_norm(qe);
            bq_rot(qe, t.t, rt);
            for (int k = 0; k < 3; ++k) t.t[k] = te[k] + rt[k];
            bq_mul(qe, t.q, qn);
            bq_norm(qn);
            std::memcpy(t.q, qn, sizeof(qn));
        }
        for (int i = 0; i < 3 * npt; ++i) X[i] = X[i] + x[n + i];
    }
    int optimize(int iters) {   // OptimizationAlgorithmLevenberg::solve, `iters` times
        double lambda = 0, ni = 2;
        int nBad = 0, it = 0;
        for (; it < iters; ++it) {
            double currentChi = errors();
            build();
            const double iniChi = currentChi;
            if (it == 0) {
                lambda = 1e-5 * max_diag();
                ni = 2;
                nBad = 0;
            }
            double rho = 0;
            int qmax = 0;
            do {
                const std::vector<BQ> Tb = T;
                const std::vector<double> Xb = X;
                const bool ok = solve(lambda);
                double tempChi;
                if (ok) {
                    update();
                    tempChi = errors();
                } else {
                    tempChi = DBL_MAX;
                }
                rho = currentChi - tempChi;
                double sc = ok ? scale(lambda) : 0.0;
                sc += 1e-3;
                rho /= sc;
                if (rho > 0 && std::isfinite(tempChi)) {
                    double alpha = 1. - std::pow((2 * rho - 1), 3);
                    alpha = std::min(alpha, 2. / 3.);
                    lambda *= std::max(1. / 3., alpha);
                    ni = 2;
                    currentChi = tempChi;
                } else {
                    lambda *= ni;
                    ni *= 2;
                    T = Tb;
                    X = Xb;
                }
                qmax++;
            } while (rho < 0 && qmax < 10);
            if (qmax == 10 || rho == 0) return it + 1;
            if ((iniChi - currentChi) * 1e3 < iniChi) nBad++;
            else nBad = 0;
            if (nBad >= 3) return it + 1;
        }
        return it;
    }
};

void oba_init(OBA &o, const float *Tcw, const uint8_t *fixed, int ncam, const float *Xw, int npt,
              const orbo_ba_edge *edges, int ne) {
    o.ncam = ncam; o.npt = npt; o.ne = ne; o.E = edges;
    o.T.resize(ncam);
    int nf = 0;
    for (int c = 0; c < ncam; ++c) {
        double R[9];
        for (int r = 0; r < 3; ++r)
            for (int k = 0; k < 3; ++k) R[3 * r + k] = Tcw[12 * (size_t)c + 4 * r + k];
        bq_fromR(R, o.T[c].q);
        bq_norm(o.T[c].q);
        for (int r = 0; r < 3; ++r) o.T[c].t[r] = Tcw[12 * (size_t)c + 4 * r + 3];
        o.T[c].f = fixed[c] ? -1 : nf++;
    }
    o.nf = nf;
    o.X.assign(Xw, Xw + 3 * (size_t)npt);
    const double thMono = (double)(float)std::sqrt(5.991), thStereo = (double)(float)std::sqrt(7.815);
    o.delta.resize(ne);
    for (int e = 0; e < ne; ++e) o.delta[e] = edges[e].ur >= 0 ? thStereo : thMono;
    o.err.assign(3 * (size_t)ne, 0); o.chi2.assign(ne, 0); o.rho0.assign(ne, 0); o.rho1.assign(ne, 0);
    o.act.assign(ne, 1); o.front.assign(ne, 0);
    o.hpp_e.assign(36 * (size_t)ne, 0); o.hll_e.assign(9 * (size_t)ne, 0); o.hpl_e.assign(18 * (size_t)ne, 0);
    o.bp_e.assign(6 * (size_t)ne, 0); o.bl_e.assign(3 * (size_t)ne, 0);
    o.pe.assign(npt, {});
    for (int e = 0; e < ne; ++e) o.pe[edges[e].point].push_back(e);
    for (auto &l : o.pe) std::stable_sort(l.begin(), l.end(), [&](int a, int b) { return edges[a].cam < edges[b].cam; });
    o.ce.assign(nf, {});
    for (int e = 0; e < ne; ++e)
        if (o.T[edges[e].cam].f >= 0) o.ce[o.T[edges[e].cam].f].push_back(e);
}
}  // namespace

int orbo_local_ba(const float *Tcw, const uint8_t *fixed, int ncam, const float *Xw, int npt,
                  const orbo_ba_edge *edges, int ne, int iters1, int iters2, float *Tcw_out, float *Xw_out,
                  uint8_t *outlier, int *iterations) {
    OBA o;
    oba_init(o, Tcw, fixed, ncam, Xw, npt, edges, ne);
    o.robust = true;
    const int it1 = o.optimize(iters1);
    int it2 = 0;
    if (iters2 > 0) {
        o.fronts();   // e->chi2() as last computed, isDepthPositive() now
        for (int e = 0; e < ne; ++e) {
            const double th = edges[e].ur >= 0 ? 7.815 : 5.991;
            if (o.chi2[e] > th || !o.front[e]) o.act[e] = 0;
        }
        o.robust = false;
        it2 = o.optimize(iters2);
    }
    o.fronts();
    for (int e = 0; e < ne; ++e) {
        const double th = edges[e].ur >= 0 ? 7.815 : 5.991;
        outlier[e] = o.chi2[e] > th || !o.front[e];
    }
    for (int c = 0; c < ncam; ++c) {
        double R[9];
        bq_R(o.T[c].q, R);
        for (int r = 0; r < 3; ++r) {
            for (int k = 0; k < 3; ++k) Tcw_out[12 * (size_t)c + 4 * r + k] = (float)R[3 * r + k];
            Tcw_out[12 * (size_t)c + 4 * r + 3] = (float)o.T[c].t[r];
        }
    }
    for (int i = 0; i < 3 * npt; ++i) Xw_out[i] = (float)o.X[i];
    if (iterations) { iterations[0] = it1; iterations[1] = it2; }
    return 0;
}

int orbo_ba_debug_step(const float *Tcw, const uint8_t *fixed, int ncam, const float *Xw, int npt,
                       const orbo_ba_edge *edges, int ne, int robust, double lambda, double *x_out, double *chi2_out) {
    OBA o;
    oba_init(o, Tcw, fixed, ncam, Xw, npt, edges, ne);
    o.robust = robust != 0;
    *chi2_out = o.errors();
    o.build();
    const bool ok = o.solve(lambda);
    if (ok) std::copy(o.x.begin(), o.x.end(), x_out);
    return ok ? 1 : 0;
}
