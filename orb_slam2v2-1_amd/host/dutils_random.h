// dutils_random.h — Thirdparty/DBoW2/DUtils/Random.cpp as the geometric solvers use it (Initializer, Sim3Solver): SeedRandOnce seeds
// rand() once per process, RandomInt scales it (:47-50).  One process-wide rand() sequence, as in the reference.
#ifndef ORBX_DUTILS_RANDOM_H
#define ORBX_DUTILS_RANDOM_H
#include <cstdlib>

namespace DUtils {
namespace Random {
inline void SeedRandOnce(int seed) {
    static bool seeded = false;   // one flag for the whole program: an inline function's static
    if (!seeded) { std::srand(seed); seeded = true; }
}
inline int RandomInt(int min, int max) {
    int d = max - min + 1;
    return int(((double)std::rand() / ((double)RAND_MAX + 1.0)) * d) + min;
}
}  // namespace Random
}  // namespace DUtils
#endif
