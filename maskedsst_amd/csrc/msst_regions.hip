// Connected regions of an integer map (msst_regions_label, msst_regions_merge; maskedsst_amd/regions.py): connected-component labelling
// of a class map or a superpixel label map [Bs][Hs][Ws] int64 on the device, and one simultaneous round of "merge the flagged regions
// into their largest neighbour" on top of it -- the sieve (minimum mapping unit) and SLIC's connectivity pass.  Integer arithmetic only:
// no float, no inline assembly, no wait on another workgroup; integer atomicMin / atomicMax / atomicAdd from plain C++.  The union, find
// and key logic is msst_regions_core.h (it also compiles into a stand-alone host program).
//
// label     three launches, whatever the map holds (Komura / Playne):
//   rg_tile     one workgroup of 256 threads per TILE of 16 x 16 pixels, thread = pixel.  The tile's values to LDS; a union-find on an
//               LDS parent array (local index = 16 ly + lx, which orders the pixels of a tile as the scene's raster order does): every
//               pixel unites with those of its BACKWARD neighbours (left, up; for 8: up-left, up-right) that lie in the tile and hold
//               its value.  Then parent[p] = the scene index of the pixel's local root, sizes[p] = the local set's pixel count at a
//               local root and 0 elsewhere, count[b] = 0.
//   rg_border   thread = pixel: the backward neighbours in ANOTHER tile with the same value are united on the global parent array.
//   rg_flatten  thread = pixel: labels[p] = find(p); a local root that is not the region's root moves its count to the root with one
//               integer atomicAdd; a root adds 1 to count[b] (summed in LDS per workgroup first).
//   A root only ever links to a smaller index, so the region's root is its smallest index -- its first pixel in raster order -- and the
//   sums are integer: the outputs do not depend on the order in which the atomics land.
// merge     three launches in mode 0, four in mode 1, thread = pixel:
//   rg_init     slots = 0; mode 1: keep = 0, the cell boxes empty.
//   rg_keep     (mode 1) per live pixel the cell box of its region (atomicMin / atomicMax at the root's entry); per root
//               atomicMax(keep[b][id], key(size, root)): the kept piece of an id.
//   rg_boundary per pixel of a flagged region R, per neighbour in a live, unflagged region T != R (mode 1: whose id is eligible for R's
//               box): atomicMax(slots[R], key(size T, root T)).  Roots count regions and flagged regions.
//   rg_apply    every pixel of a flagged region with a non-zero slot takes the value at the winner's root pixel.  Roots count merged
//               regions, pixels count changed pixels.
//   Every decision reads the round's input (values, labels, sizes) and the slots, never values_out: the round is simultaneous.
#include "../../include/msst.h"
#include "msst_kernels.h"
#include "msst_regions_core.h"

namespace msst {

namespace {

constexpr int RG_T = 16;                       // the tile's side
constexpr int RG_ERR_BYTES = 16;               // the error word and its padding at the head of the scratch

struct RgGeo {
    int Bs, Hs, Ws, nty, ntx, conn;
    __host__ __device__ long plane() const { return (long)Hs * Ws; }
    __host__ __device__ long tiles() const { return (long)Bs * nty * ntx; }
};

RgGeo rg_geo(int Bs, int Hs, int Ws, int conn) {
    RgGeo g;
    g.Bs = Bs; g.Hs = Hs; g.Ws = Ws; g.conn = conn;
    g.nty = (Hs + RG_T - 1) / RG_T; g.ntx = (Ws + RG_T - 1) / RG_T;
    return g;
}

struct RgTile {
    int b, y, x, ly, lx;
    bool in;
    long p;       // b plane + i
    int i;        // y Ws + x
};

__device__ __forceinline__ RgTile rg_tile_of(const RgGeo& g) {
    RgTile k;
    int t = blockIdx.x;
    const int tx = t % g.ntx;
    t /= g.ntx;
    const int ty = t % g.nty;
    k.b = t / g.nty;
    k.ly = threadIdx.x >> 4; k.lx = threadIdx.x & 15;
    k.y = ty * RG_T + k.ly; k.x = tx * RG_T + k.lx;
    k.in = k.y < g.Hs && k.x < g.Ws;
    k.i = k.in ? k.y * g.Ws + k.x : 0;
    k.p = (long)k.b * g.plane() + k.i;
    return k;
}

__global__ __launch_bounds__(256) void rg_tile_kernel(const int64_t* __restrict__ values, int* parent, int32_t* sizes, int32_t* count, int* err,
                                                      RgGeo g) {
    __shared__ long long sv[RG_T * RG_T];
    __shared__ int L[RG_T * RG_T];
    __shared__ int cnt[RG_T * RG_T];
    const int tid = threadIdx.x;
    const RgTile k = rg_tile_of(g);
    const long long v = k.in ? (long long)values[k.p] : -1;
    const bool live = v >= 0;
    sv[tid] = v;
    L[tid] = live ? tid : -1;
    cnt[tid] = 0;
    __syncthreads();
    int hit = 0;
    if (live) {
        const int nb = rg_back_count(g.conn);
        for (int n = 0; n < nb; ++n) {
            const int ny = k.ly + rg_back_dy(n), nx = k.lx + rg_back_dx(n);
            if (ny < 0 || nx < 0 || nx >= RG_T) continue;
            const int q = ny * RG_T + nx;
            if (sv[q] == v) rg_union(L, tid, q, RG_T * RG_T, &hit);
        }
    }
    __syncthreads();
    int r = tid;
    if (live) {
        r = rg_find(L, tid, RG_T * RG_T, &hit);
        atomicAdd(&cnt[r], 1);
    }
    __syncthreads();
    if (k.in) {
        parent[k.p] = live ? (k.y - k.ly + (r >> 4)) * g.Ws + (k.x - k.lx + (r & 15)) : -1;
        sizes[k.p] = live ? cnt[tid] : 0;      // non-zero at a local root only
    }
    if (tid == 0 && blockIdx.x % (g.nty * g.ntx) == 0) count[k.b] = 0;
    if (hit) atomicMax(err, hit);
}

__global__ __launch_bounds__(256) void rg_border_kernel(const int64_t* __restrict__ values, int* parent, int* err, RgGeo g) {
    const RgTile k = rg_tile_of(g);
    if (!k.in || (k.ly > 0 && k.lx > 0 && k.lx < RG_T - 1)) return;    // an interior pixel has no backward neighbour in another tile
    const long base = (long)k.b * g.plane();
    const int64_t v = values[k.p];
    if (v < 0) return;
    int hit = 0;
    const int nb = rg_back_count(g.conn);
    for (int n = 0; n < nb; ++n) {
        const int ny = k.y + rg_back_dy(n), nx = k.x + rg_back_dx(n);
        if (ny < 0 || nx < 0 || nx >= g.Ws) continue;
        if (ny / RG_T == k.y / RG_T && nx / RG_T == k.x / RG_T) continue;      // the tile kernel did this pair
        const int q = ny * g.Ws + nx;
        if (values[base + q] == v) rg_union(parent + base, k.i, q, g.plane(), &hit);
    }
    if (hit) atomicMax(err, hit);
}

__global__ __launch_bounds__(256) void rg_flatten_kernel(const int* parent, int64_t* labels, int32_t* sizes, int32_t* count, int* err, long plane,
                                                         long total) {
    __shared__ int nroots;
    if (threadIdx.x == 0) nroots = 0;
    __syncthreads();
    const long first = (long)blockIdx.x * 256;
    const long e = first + threadIdx.x;
    const int b0 = (int)(first / plane);
    if (e < total) {
        const int b = (int)(e / plane);
        const int i = (int)(e - (long)b * plane);
        const long base = (long)b * plane;
        if (parent[e] < 0) {
            labels[e] = -1;
        } else {
            int hit = 0;
            const int r = rg_find(parent + base, i, plane, &hit);
            labels[e] = r;
            if (r != i) {
                const int c = sizes[e];        // nobody adds to the entry of a pixel that is not its region's root
                if (c) {
                    sizes[e] = 0;
                    atomicAdd(&sizes[base + r], c);
                }
            } else if (b == b0) {
                atomicAdd(&nroots, 1);
            } else {
                atomicAdd(&count[b], 1);
            }
            if (hit) atomicMax(err, hit);
        }
    }
    __syncthreads();
    if (threadIdx.x == 0 && nroots) atomicAdd(&count[b0], nroots);
}

// ------------------------------------------------------------------------------------------------------------------------- merge
struct RgMergeArgs {
    const int64_t* values;
    const int64_t* labels;
    const int32_t* sizes;
    int64_t* out;
    int32_t* history;                // regions, flagged, merged, changed
    unsigned long long* slots;       // [Bs plane], read at a root
    unsigned long long* keep;        // [Bs n_sp] (mode 1)
    int* box;                        // [Bs plane][4]: i0, i1, j0, j1 at a root (mode 1)
    int Bs, Hs, Ws, conn, mode, min_size, S, gx, n_sp;
    __host__ __device__ long plane() const { return (long)Hs * Ws; }
};

struct RgPixel {
    int b, i, y, x;
    long base;
    bool ok;
};

__device__ __forceinline__ RgPixel rg_pixel(const RgMergeArgs& a) {
    RgPixel k;
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    const long plane = a.plane();
    k.ok = e < (long)a.Bs * plane;
    k.b = k.ok ? (int)(e / plane) : 0;
    k.base = (long)k.b * plane;
    k.i = k.ok ? (int)(e - k.base) : 0;
    k.y = k.i / a.Ws;
    k.x = k.i - k.y * a.Ws;
    return k;
}

__device__ __forceinline__ bool rg_live(const RgMergeArgs& a, int64_t v) { return v >= 0 && (a.mode == 0 || v < a.n_sp); }

// the root of pixel q (an index into the batch) as the labelling wrote it; -1 for an entry that is no index of the scene (labels that
// do not come from msst_regions_label): such a pixel is treated as dead, nothing is read through it
__device__ __forceinline__ int rg_root(const RgMergeArgs& a, long q) {
    const int64_t r = a.labels[q];
    return r >= 0 && r < a.plane() ? (int)r : -1;
}

// is the live region of value v, root r (scene b) flagged?
__device__ __forceinline__ bool rg_flagged(const RgMergeArgs& a, int b, int64_t v, int r, int size) {
    if (a.mode == 0) return size < a.min_size;
    return a.keep[(long)b * a.n_sp + v] != rg_key(size, r);
}

__global__ __launch_bounds__(256) void rg_init_kernel(RgMergeArgs a) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= (long)a.Bs * a.plane()) return;
    a.slots[e] = 0;
    if (a.mode == 1) {
        if (e < (long)a.Bs * a.n_sp) a.keep[e] = 0;
        a.box[4 * e] = 0x7fffffff; a.box[4 * e + 1] = -1; a.box[4 * e + 2] = 0x7fffffff; a.box[4 * e + 3] = -1;
    }
}

__global__ __launch_bounds__(256) void rg_keep_kernel(RgMergeArgs a) {
    const RgPixel k = rg_pixel(a);
    if (!k.ok) return;
    const int64_t v = a.values[k.base + k.i];
    if (!rg_live(a, v)) return;
    const int r = rg_root(a, k.base + k.i);
    if (r < 0) return;
    int* box = a.box + 4 * (k.base + r);
    const int ci = k.y / a.S, cj = k.x / a.S;
    if (rg_load(box) > ci) atomicMin(box, ci);              // a stale read only costs an atomic: the entries move one way
    if (rg_load(box + 1) < ci) atomicMax(box + 1, ci);
    if (rg_load(box + 2) > cj) atomicMin(box + 2, cj);
    if (rg_load(box + 3) < cj) atomicMax(box + 3, cj);
    if (r == k.i) atomicMax(a.keep + (long)k.b * a.n_sp + v, rg_key(a.sizes[k.base + r], r));
}

__device__ __forceinline__ void rg_history_add(int* sh, int32_t* history, int n0, int n1, int at) {
    // sh: two LDS counters zeroed before the barrier that precedes the adds
    if (n0) atomicAdd(&sh[0], n0);
    if (n1) atomicAdd(&sh[1], n1);
    __syncthreads();
    if (threadIdx.x < 2 && sh[threadIdx.x]) atomicAdd(&history[at + threadIdx.x], sh[threadIdx.x]);
}

__global__ __launch_bounds__(256) void rg_boundary_kernel(RgMergeArgs a) {
    __shared__ int sh[2];
    if (threadIdx.x < 2) sh[threadIdx.x] = 0;
    __syncthreads();
    const RgPixel k = rg_pixel(a);
    int nreg = 0, nflag = 0;
    if (k.ok) {
        const int64_t v = a.values[k.base + k.i];
        const int r = rg_live(a, v) ? rg_root(a, k.base + k.i) : -1;
        if (r >= 0) {
            const bool flagged = rg_flagged(a, k.b, v, r, a.sizes[k.base + r]);
            if (r == k.i) {
                nreg = 1;
                nflag = flagged ? 1 : 0;
            }
            if (flagged) {
                unsigned long long best = 0;
                int bx[4] = {0, 0, 0, 0};
                if (a.mode == 1) {
                    for (int c = 0; c < 4; ++c) bx[c] = a.box[4 * (k.base + r) + c];
                }
                for (int n = 0; n < a.conn; ++n) {
                    const int ny = k.y + rg_dy(n), nx = k.x + rg_dx(n);
                    if (ny < 0 || ny >= a.Hs || nx < 0 || nx >= a.Ws) continue;
                    const long q = k.base + (long)ny * a.Ws + nx;
                    const int64_t vq = a.values[q];
                    if (!rg_live(a, vq)) continue;
                    const int rq = rg_root(a, q);
                    if (rq < 0 || rq == r) continue;
                    const int sq = a.sizes[k.base + rq];
                    if (rg_flagged(a, k.b, vq, rq, sq)) continue;
                    if (a.mode == 1 && !rg_eligible((int)vq, a.gx, bx[0], bx[1], bx[2], bx[3])) continue;
                    const unsigned long long key = rg_key(sq, rq);
                    if (key > best) best = key;
                }
                if (best) atomicMax(a.slots + k.base + r, best);
            }
        }
    }
    rg_history_add(sh, a.history, nreg, nflag, 0);
}

__global__ __launch_bounds__(256) void rg_apply_kernel(RgMergeArgs a) {
    __shared__ int sh[2];
    if (threadIdx.x < 2) sh[threadIdx.x] = 0;
    __syncthreads();
    const RgPixel k = rg_pixel(a);
    int nmerged = 0, nchanged = 0;
    if (k.ok) {
        const int64_t v = a.values[k.base + k.i];
        int64_t out = v;
        const int r = rg_live(a, v) ? rg_root(a, k.base + k.i) : -1;
        if (r >= 0) {
            if (rg_flagged(a, k.b, v, r, a.sizes[k.base + r])) {
                const unsigned long long key = a.slots[k.base + r];
                if (key) {
                    out = a.values[k.base + rg_key_root(key)];
                    nchanged = out != v ? 1 : 0;
                    nmerged = r == k.i ? 1 : 0;
                }
            }
        }
        a.out[k.base + k.i] = out;
    }
    rg_history_add(sh, a.history, nmerged, nchanged, 2);
}

}  // namespace

long regions_tiles(int Bs, int Hs, int Ws) { return (long)Bs * ((Hs + RG_T - 1) / RG_T) * ((Ws + RG_T - 1) / RG_T); }

// the error word | the larger of: parent (int32 per pixel) and slots, keep (64 bits per pixel each) with the boxes (4 int32 per pixel)
long regions_scratch_bytes(int Bs, int Hs, int Ws) { return RG_ERR_BYTES + 32L * Bs * Hs * Ws; }

int launch_regions_label(const int64_t* values, int Bs, int Hs, int Ws, int connectivity, int64_t* labels, int32_t* sizes, int32_t* count,
                         void* scratch, hipStream_t st) {
    const RgGeo g = rg_geo(Bs, Hs, Ws, connectivity);
    int* err = (int*)scratch;
    int* parent = (int*)((char*)scratch + RG_ERR_BYTES);
    const long total = (long)Bs * g.plane();
    hipLaunchKernelGGL(rg_tile_kernel, dim3((unsigned)g.tiles()), dim3(256), 0, st, values, parent, sizes, count, err, g);
    hipLaunchKernelGGL(rg_border_kernel, dim3((unsigned)g.tiles()), dim3(256), 0, st, values, parent, err, g);
    hipLaunchKernelGGL(rg_flatten_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, parent, labels, sizes, count, err, g.plane(),
                       total);
    return (int)hipGetLastError();
}

int launch_regions_merge(const int64_t* values, const int64_t* labels, const int32_t* sizes, int Bs, int Hs, int Ws, int connectivity, int mode,
                         int min_size, int step, int64_t* values_out, int32_t* history, void* scratch, hipStream_t st) {
    RgMergeArgs a;
    const long total = (long)Bs * Hs * Ws;
    a.values = values; a.labels = labels; a.sizes = sizes; a.out = values_out; a.history = history;
    a.slots = (unsigned long long*)((char*)scratch + RG_ERR_BYTES);
    a.keep = a.slots + total;
    a.box = (int*)(a.keep + total);
    a.Bs = Bs; a.Hs = Hs; a.Ws = Ws; a.conn = connectivity; a.mode = mode; a.min_size = min_size;
    a.S = mode == 1 ? step : 1;
    a.gx = (Ws + a.S - 1) / a.S;
    a.n_sp = mode == 1 ? ((Hs + a.S - 1) / a.S) * a.gx : 0;
    const dim3 grid((unsigned)((total + 255) / 256));
    hipLaunchKernelGGL(rg_init_kernel, grid, dim3(256), 0, st, a);
    if (mode == 1) hipLaunchKernelGGL(rg_keep_kernel, grid, dim3(256), 0, st, a);
    hipLaunchKernelGGL(rg_boundary_kernel, grid, dim3(256), 0, st, a);
    hipLaunchKernelGGL(rg_apply_kernel, grid, dim3(256), 0, st, a);
    return (int)hipGetLastError();
}

}  // namespace msst
