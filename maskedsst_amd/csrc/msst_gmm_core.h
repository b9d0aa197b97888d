// The factorisation Sigma = L L^T and the triangular inverse A = L^-1 of msst_gmm.hip (msst_gmm_update) as plain functions on doubles:
// no float, no atomics, no inline assembly.  The same text compiles for the device (hipcc) and for a stand-alone host program (any
// C++17 compiler; tools/gmm_core_check.cpp), which is where a CPU sanitizer run belongs.
//
// Both functions are written for a team of `nt` workers: worker `tid` does its share and `sync()` is the team's barrier (on the device
// 256 threads and __syncthreads; on the host tid = 0, nt = 1 and a sync that does nothing).  Every entry is written by exactly one
// worker and every sum runs in one fixed order, so the result does not depend on nt.  Every loop has a trip count fixed by n: no
// loop waits for a value.  A decision that ends a function early is made by every worker from the same stored value after a barrier,
// so the team leaves together.
//   a         [n][pitch] doubles, row-major; only the lower triangle (j <= i) is read or written.
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#define GMM_HD __host__ __device__ __forceinline__
#else
#define GMM_HD inline
#endif

namespace msst {

// a (lower triangle of a symmetric matrix) -> L in place, right-looking, column by column.  false: column j met a pivot that is not
// finite or not positive (a is then half factorised and of no use); *logdet = 2 sum_j log L[j][j], summed in j order by every worker
template <class Sync>
GMM_HD bool gmm_cholesky(double* a, int n, int pitch, int tid, int nt, Sync&& sync, double* logdet) {
    double ld = 0.0;
    const int tw = nt % 16 == 0 ? 16 : 1, th = nt / tw, ti = tid / tw, tk = tid % tw;
    for (int j = 0; j < n; ++j) {
        sync();                                   // the trailing update of column j - 1 is done
        const double d = a[j * pitch + j];
        if (!(d > 0.0) || !(d <= 1.7976931348623157e308)) return false;
        const double l = sqrt(d);
        ld += log(l);
        sync();                                   // every worker has read the pivot
        if (tid == 0) a[j * pitch + j] = l;
        for (int i = j + 1 + tid; i < n; i += nt) a[i * pitch + j] /= l;
        sync();
        // the trailing update: the team as th x tw workers, worker (ti, tk) on rows i = j + 1 + ti + th u and columns k = j + 1 + tk + tw v
        for (int i = j + 1 + ti; i < n; i += th) {
            const double lij = a[i * pitch + j];
            for (int k = j + 1 + tk; k <= i; k += tw) a[i * pitch + k] -= lij * a[k * pitch + j];
        }
    }
    sync();
    *logdet = 2.0 * ld;
    return true;
}

// L (lower triangular, a positive diagonal) -> A = L^-1 in place, row by row: A[i][i] = 1 / L[i][i], A[i][j] = -(sum_{k = j}^{i - 1}
// L[i][k] A[k][j]) / L[i][i], the sum in one fixed order (below).  row: n doubles of scratch shared by the team
template <class Sync>
GMM_HD void gmm_tri_inverse(double* a, int n, int pitch, double* row, int tid, int nt, Sync&& sync) {
    for (int i = 0; i < n; ++i) {
        sync();                                   // row i - 1 is written
        for (int k = tid; k <= i; k += nt) row[k] = a[i * pitch + k];
        sync();
        const double inv = 1.0 / row[i];
        for (int j = tid; j <= i; j += nt) {
            if (j == i) {
                a[i * pitch + i] = inv;
            } else {   // four interleaved partial sums (k = j + 4 u + v), joined as (s0 + s1) + (s2 + s3): four chains in flight, one order
                double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
                int k = j;
                for (; k + 3 < i; k += 4) {
                    s0 += row[k] * a[k * pitch + j];
                    s1 += row[k + 1] * a[(k + 1) * pitch + j];
                    s2 += row[k + 2] * a[(k + 2) * pitch + j];
                    s3 += row[k + 3] * a[(k + 3) * pitch + j];
                }
                if (k < i) s0 += row[k] * a[k * pitch + j];
                if (k + 1 < i) s1 += row[k + 1] * a[(k + 1) * pitch + j];
                if (k + 2 < i) s2 += row[k + 2] * a[(k + 2) * pitch + j];
                a[i * pitch + j] = -((s0 + s1) + (s2 + s3)) * inv;
            }
        }
    }
    sync();
}

}  // namespace msst
