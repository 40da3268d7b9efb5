// Test stand-in for Thirdparty/DBoW2/DUtils/Random.h: RandomInt over a small
// linear congruential generator the test can replay (x <- 1103515245 x + 12345
// mod 2^31, the draw is min + x mod (max - min + 1)), counting its calls.
#pragma once
#include <cstdint>

namespace DUtils {
namespace Random {

inline uint32_t &State() {
    static uint32_t x = 12345;
    return x;
}
inline int &Calls() {
    static int n = 0;
    return n;
}
inline int RandomInt(int min, int max) {
    uint32_t &x = State();
    x = (1103515245u * x + 12345u) & 0x7fffffffu;
    ++Calls();
    return min + (int)(x % (uint32_t)(max - min + 1));
}

}  // namespace Random
}  // namespace DUtils
