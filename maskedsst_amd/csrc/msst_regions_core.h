// The union, find and merge-key logic of msst_regions.hip as plain functions: integer only, no float, no inline assembly.  The same text
// compiles for the device (hipcc) and for a stand-alone host program (any C++17 compiler; tools/regions_core_check.cpp), which is where a
// CPU sanitizer run belongs.
//
// parent    int32 per pixel, an index within its scene (or within its tile, in LDS); -1 for a dead pixel.  INVARIANT: parent[i] <= i.
//           A link is only ever made from a root to a smaller index (rg_union: integer atomicMin), so a value only decreases, and the
//           smallest index of a set can never get a parent other than itself: when all unions are done the root of a set is its
//           smallest index, whatever order the atomics landed in.
// caps      rg_find follows strictly decreasing indices: at most `cap` steps for cap >= the number of pixels.  Every turn of rg_union's
//           loop either ends it or lowers one of the two indices it holds: at most 2 x pixels turns.  Both loops still count their
//           turns against `cap` and report a hit through *hit instead of going on: a bug shows as an error word, never as a hang.
// key       (size << 32) | (0xFFFFFFFF - root): the larger key is the region of larger size, then of lower root; 0 is "none" (a size
//           is at least 1).  One 64-bit integer atomicMax picks the winner, and the same key picks the kept piece of a superpixel.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define RG_HD __host__ __device__ __forceinline__
#else
#define RG_HD inline
#endif

namespace msst {

constexpr int RG_ERR_FIND_CAP = 1;     // error word: rg_find ran into its cap
constexpr int RG_ERR_UNION_CAP = 2;    // error word: rg_union ran into its cap

RG_HD int rg_load(const int* p) { return __atomic_load_n(p, __ATOMIC_RELAXED); }

// atomicMin on the device; in the stand-alone host program the same contract through the compiler's builtin compare-exchange
RG_HD int rg_atomic_min(int* p, int v) {
#if defined(__HIP_DEVICE_COMPILE__)
    return atomicMin(p, v);
#else
    int old = __atomic_load_n(p, __ATOMIC_RELAXED);
    while (old > v && !__atomic_compare_exchange_n(p, &old, v, false, __ATOMIC_RELAXED, __ATOMIC_RELAXED)) {}
    return old;
#endif
}

// the root of i: follow the parents while they decrease.  i is live (parent[i] >= 0)
RG_HD int rg_find(const int* parent, int i, long long cap, int* hit) {
    int p = rg_load(parent + i);
    long long n = 0;
    while (p != i) {
        if (p < 0 || p > i || ++n > cap) {   // a broken invariant is reported like a cap
            *hit |= RG_ERR_FIND_CAP;
            return i;
        }
        i = p;
        p = rg_load(parent + i);
    }
    return i;
}

// unite the sets of a and b (Playne and Hawick's lock-free union): link the larger root to the smaller with atomicMin; when another
// thread linked that root first, go on from where it points
RG_HD void rg_union(int* parent, int a, int b, long long cap, int* hit) {
    for (long long n = 0;; ++n) {
        if (n > 2 * cap) {
            *hit |= RG_ERR_UNION_CAP;
            return;
        }
        a = rg_find(parent, a, cap, hit);
        b = rg_find(parent, b, cap, hit);
        if (*hit || a == b) return;
        if (a < b) {
            const int t = a;
            a = b;
            b = t;
        }
        const int old = rg_atomic_min(parent + a, b);   // a > b
        if (old == a) return;
        a = old;
    }
}

RG_HD unsigned long long rg_key(int size, int root) {
    return ((unsigned long long)(unsigned)size << 32) | (unsigned long long)(0xFFFFFFFFu - (unsigned)root);
}
RG_HD int rg_key_root(unsigned long long key) { return (int)(0xFFFFFFFFu - (unsigned)(key & 0xFFFFFFFFull)); }
RG_HD int rg_key_size(unsigned long long key) { return (int)(key >> 32); }

// mode 1: may a piece whose pixels lie in the cells [i0, i1] x [j0, j1] take the superpixel id m of a grid gx cells wide?  Yes when
// every one of those cells lies in the 3 x 3 cells around m's own: the invariant msst_slic_pool relies on.
RG_HD bool rg_eligible(int m, int gx, int i0, int i1, int j0, int j1) {
    const int im = m / gx, jm = m - im * gx;
    return im - 1 <= i0 && i1 <= im + 1 && jm - 1 <= j0 && j1 <= jm + 1;
}

// the neighbours of a pixel: the first 4 are the cross (left, up, right, down), the other 4 the diagonals; connectivity = how many
// are walked.  The first RG_BACK(connectivity) entries of rg_back_* are the neighbours that come before a pixel in raster order.
RG_HD int rg_dy(int k) { return k == 1 ? -1 : k == 3 ? 1 : k == 4 || k == 5 ? -1 : k >= 6 ? 1 : 0; }
RG_HD int rg_dx(int k) { return k == 0 ? -1 : k == 2 ? 1 : k == 4 || k == 6 ? -1 : k == 5 || k == 7 ? 1 : 0; }
RG_HD int rg_back_dy(int k) { return k == 0 ? 0 : -1; }                 // left, up, up-left, up-right
RG_HD int rg_back_dx(int k) { return k == 0 ? -1 : k == 1 ? 0 : k == 2 ? -1 : 1; }
RG_HD int rg_back_count(int connectivity) { return connectivity == 8 ? 4 : 2; }

}  // namespace msst
