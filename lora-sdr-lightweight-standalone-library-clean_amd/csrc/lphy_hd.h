// lphy_hd.h — LPHY_HD, in front of what both the kernels and the host call:
// host and device under hipcc, plain C++ for a CPU test that compiles the
// header alone.
#pragma once

#if defined(__HIPCC__)
#define LPHY_HD __host__ __device__ __forceinline__
#else
#define LPHY_HD inline
#endif
