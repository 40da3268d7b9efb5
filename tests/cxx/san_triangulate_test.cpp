// Stand-alone ASan + UBSan driver of the host validation of
// orbx_triangulate / orbx_triangulate_batch (orbx_triangulate.hip compiled with
// -Xarch_host -fsanitize=address,undefined; tests/test_triangulate_sanitizer.py).
// Every call here returns before the library touches a device: the validation
// walks offsets[0 .. nproblems] and pairs[0 .. offsets[nproblems]) of
// exact-size heap arrays to their last element, so a read past either end is
// a sanitizer report.  No GPU is needed and none is used.
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "orbx.h"

static int fails = 0;
#define CHECK(cond)                                             \
    do {                                                        \
        if (!(cond)) {                                          \
            std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #cond); \
            ++fails;                                            \
        }                                                       \
    } while (0)

static orbx_tri_obs mono(float u) {
    orbx_tri_obs o;
    std::memset(&o, 0, sizeof(o));
    o.u = u; o.v = 2 * u; o.ur = -1.0f; o.depth = -1.0f; o.raw_u = u; o.raw_v = 2 * u; o.sigma2 = 1.0f; o.scale = 1.0f;
    return o;
}

int main() {
    const int P = 5;
    std::vector<orbx_tri_view> v1(P), v2(P);
    std::memset(v1.data(), 0, sizeof(orbx_tri_view) * P);
    std::memset(v2.data(), 0, sizeof(orbx_tri_view) * P);
    std::vector<float> rf(P, 1.8f);
    const std::vector<int32_t> good = {0, 0, 70, 70, 131, 131};   // empty problems first, inside and last
    std::vector<orbx_tri_pair> pairs(131);
    for (size_t i = 0; i < pairs.size(); ++i) pairs[i].o1 = mono((float)i), pairs[i].o2 = mono(0.5f * i);
    std::vector<orbx_tri_point> out(131);

    // negative sizes
    CHECK(orbx_triangulate(0, v1.data(), v2.data(), 1.8f, pairs.data(), -1, out.data()) == ORBX_EINVAL);
    CHECK(orbx_triangulate_batch(0, v1.data(), v2.data(), rf.data(), pairs.data(), good.data(), -1, out.data()) ==
          ORBX_EINVAL);
    // nothing to do: legal, nothing read or written (null arrays)
    CHECK(orbx_triangulate_batch(0, nullptr, nullptr, nullptr, nullptr, nullptr, 0, nullptr) == ORBX_OK);
    CHECK(orbx_triangulate(0, v1.data(), v2.data(), 1.8f, nullptr, 0, nullptr) == ORBX_OK);
    const std::vector<int32_t> zeros(P + 1, 0);
    CHECK(orbx_triangulate_batch(0, v1.data(), v2.data(), rf.data(), nullptr, zeros.data(), P, nullptr) == ORBX_OK);
    // offsets: not starting at 0, descending in the middle, descending at the very last entry, negative
    for (const std::vector<int32_t> &off : {std::vector<int32_t>{1, 1, 70, 70, 131, 131},
                                            std::vector<int32_t>{0, 0, 70, 69, 131, 131},
                                            std::vector<int32_t>{0, 0, 70, 70, 131, 130},
                                            std::vector<int32_t>{0, -1, 70, 70, 131, 131}})
        CHECK(orbx_triangulate_batch(0, v1.data(), v2.data(), rf.data(), pairs.data(), off.data(), P, out.data()) ==
              ORBX_EINVAL);
    // null arrays with work to do
    CHECK(orbx_triangulate_batch(0, v1.data(), v2.data(), rf.data(), nullptr, good.data(), P, out.data()) == ORBX_EINVAL);
    CHECK(orbx_triangulate_batch(0, v1.data(), v2.data(), rf.data(), pairs.data(), good.data(), P, nullptr) ==
          ORBX_EINVAL);
    CHECK(orbx_triangulate_batch(0, nullptr, v2.data(), rf.data(), pairs.data(), good.data(), P, out.data()) ==
          ORBX_EINVAL);
    // the invalid stereo depth on either side, at the first and at the very last pair: zero, negative, NaN
    const float bad_depth[3] = {0.0f, -2.0f, std::numeric_limits<float>::quiet_NaN()};
    for (size_t where : {size_t(0), pairs.size() - 1})
        for (int side = 0; side < 2; ++side)
            for (float d : bad_depth) {
                std::vector<orbx_tri_pair> k(pairs);
                orbx_tri_obs &o = side ? k[where].o2 : k[where].o1;
                o.ur = side ? 0.0f : 100.0f;
                o.depth = d;
                CHECK(orbx_triangulate_batch(0, v1.data(), v2.data(), rf.data(), k.data(), good.data(), P,
                                             out.data()) == ORBX_EINVAL);
                if (where == 0)
                    CHECK(orbx_triangulate(0, v1.data(), v2.data(), 1.8f, k.data(), 1, out.data()) == ORBX_EINVAL);
            }
    // the _device entry's own argument checks (no launch: a bad count, nothing to do, a null array)
    CHECK(orbx_triangulate_batch_device(nullptr, nullptr, nullptr, nullptr, nullptr, -1, 0, nullptr, nullptr) ==
          ORBX_EINVAL);
    CHECK(orbx_triangulate_batch_device(nullptr, nullptr, nullptr, nullptr, nullptr, 3, -1, nullptr, nullptr) ==
          ORBX_EINVAL);
    CHECK(orbx_triangulate_batch_device(nullptr, nullptr, nullptr, nullptr, nullptr, 0, 0, nullptr, nullptr) == ORBX_OK);
    CHECK(orbx_triangulate_batch_device(nullptr, nullptr, nullptr, nullptr, nullptr, 3, 0, nullptr, nullptr) == ORBX_OK);
    CHECK(orbx_triangulate_batch_device(nullptr, nullptr, nullptr, nullptr, nullptr, 3, 5, nullptr, nullptr) ==
          ORBX_EINVAL);
    if (fails) return 1;
    std::printf("sanitize triangulate ok\n");
    return 0;
}
