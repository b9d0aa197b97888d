// A stand-alone host program over maskedsst_amd/csrc/msst_regions_core.h: the union, find and key functions of msst_regions.hip run on
// the CPU in the kernel's three steps (a union-find per 16 x 16 tile, unions across the tile borders, a flatten that counts sizes), with
// the pixels of every step visited in a shuffled order, from several threads, against a flood fill.  This is where a sanitizer belongs:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -pthread tools/regions_core_check.cpp -o regions_core_check && ./regions_core_check
//   c++ -std=c++17 -O1 -g -fsanitize=thread -pthread tools/regions_core_check.cpp -o regions_core_check_tsan && ./regions_core_check_tsan
// It is not part of the test suite.  Exit status 0 and "ok" when every case agrees.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <numeric>
#include <random>
#include <thread>
#include <vector>

#include "../maskedsst_amd/csrc/msst_regions_core.h"

using namespace msst;

static const int T = 16;

struct Map {
    int H, W;
    std::vector<long long> v;
};

static void flood(const Map& m, int conn, std::vector<int>& label, std::vector<int>& size) {
    const int n = m.H * m.W;
    label.assign(n, -1);
    size.assign(n, 0);
    std::vector<int> stack;
    for (int s = 0; s < n; ++s) {
        if (m.v[s] < 0 || label[s] >= 0) continue;
        label[s] = s;
        stack.assign(1, s);
        int cnt = 0;
        while (!stack.empty()) {
            const int p = stack.back();
            stack.pop_back();
            ++cnt;
            for (int k = 0; k < conn; ++k) {
                const int y = p / m.W + rg_dy(k), x = p % m.W + rg_dx(k);
                if (y < 0 || y >= m.H || x < 0 || x >= m.W) continue;
                const int q = y * m.W + x;
                if (m.v[q] == m.v[p] && label[q] < 0) {
                    label[q] = s;
                    stack.push_back(q);
                }
            }
        }
        size[s] = cnt;
    }
}

template <class F>
static void shuffled_parallel(int n, unsigned seed, int threads, F f) {
    std::vector<int> order(n);
    std::iota(order.begin(), order.end(), 0);
    std::mt19937 rng(seed);
    std::shuffle(order.begin(), order.end(), rng);
    std::vector<std::thread> pool;
    for (int t = 0; t < threads; ++t)
        pool.emplace_back([&, t] {
            for (int i = t; i < n; i += threads) f(order[i]);
        });
    for (auto& th : pool) th.join();
}

static int run(const Map& m, int conn, unsigned seed, int threads) {
    const int n = m.H * m.W;
    const long long cap = n;
    std::vector<int> parent(n), sizes(n, 0), label(n);
    // step 1: per tile, on indices local to the tile (as the kernel's LDS array), then written out as scene indices
    for (int ty = 0; ty < (m.H + T - 1) / T; ++ty)
        for (int tx = 0; tx < (m.W + T - 1) / T; ++tx) {
            int L[T * T], cnt[T * T] = {0};
            long long sv[T * T];
            for (int l = 0; l < T * T; ++l) {
                const int y = ty * T + l / T, x = tx * T + l % T;
                sv[l] = y < m.H && x < m.W ? m.v[y * m.W + x] : -1;
                L[l] = sv[l] >= 0 ? l : -1;
            }
            int hit = 0;
            shuffled_parallel(T * T, seed + 7 * ty + tx, threads, [&](int l) {
                if (sv[l] < 0) return;
                int h = 0;
                for (int k = 0; k < rg_back_count(conn); ++k) {
                    const int ny = l / T + rg_back_dy(k), nx = l % T + rg_back_dx(k);
                    if (ny < 0 || nx < 0 || nx >= T) continue;
                    if (sv[ny * T + nx] == sv[l]) rg_union(L, l, ny * T + nx, T * T, &h);
                }
                if (h) __atomic_fetch_or(&hit, h, __ATOMIC_RELAXED);
            });
            for (int l = 0; l < T * T; ++l)
                if (sv[l] >= 0) ++cnt[rg_find(L, l, T * T, &hit)];
            for (int l = 0; l < T * T; ++l) {
                const int y = ty * T + l / T, x = tx * T + l % T;
                if (y >= m.H || x >= m.W) continue;
                const int r = sv[l] >= 0 ? rg_find(L, l, T * T, &hit) : -1;
                parent[y * m.W + x] = r < 0 ? -1 : (ty * T + r / T) * m.W + tx * T + r % T;
                sizes[y * m.W + x] = sv[l] >= 0 ? cnt[l] : 0;
            }
            if (hit) return 100 + hit;
        }
    // step 2: the backward neighbours in another tile
    int hit = 0;
    shuffled_parallel(n, seed + 1, threads, [&](int p) {
        if (m.v[p] < 0) return;
        const int y = p / m.W, x = p % m.W;
        int h = 0;
        for (int k = 0; k < rg_back_count(conn); ++k) {
            const int ny = y + rg_back_dy(k), nx = x + rg_back_dx(k);
            if (ny < 0 || nx < 0 || nx >= m.W) continue;
            if (ny / T == y / T && nx / T == x / T) continue;
            if (m.v[ny * m.W + nx] == m.v[p]) rg_union(parent.data(), p, ny * m.W + nx, cap, &h);
        }
        if (h) __atomic_fetch_or(&hit, h, __ATOMIC_RELAXED);
    });
    if (hit) return 200 + hit;
    // step 3: flatten and count
    shuffled_parallel(n, seed + 2, threads, [&](int p) {
        if (parent[p] < 0) {
            label[p] = -1;
            return;
        }
        int h = 0;
        const int r = rg_find(parent.data(), p, cap, &h);
        label[p] = r;
        if (r != p) {
            const int c = sizes[p];
            if (c) {
                sizes[p] = 0;
                __atomic_fetch_add(&sizes[r], c, __ATOMIC_RELAXED);
            }
        }
        if (h) __atomic_fetch_or(&hit, h, __ATOMIC_RELAXED);
    });
    if (hit) return 300 + hit;
    std::vector<int> want, wsize;
    flood(m, conn, want, wsize);
    for (int p = 0; p < n; ++p)
        if (label[p] != want[p] || __atomic_load_n(&sizes[p], __ATOMIC_RELAXED) != wsize[p]) return 1;
    return 0;
}

static Map make(int H, int W, int kind, unsigned seed) {
    Map m{H, W, std::vector<long long>((size_t)H * W)};
    std::mt19937 rng(seed);
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
            long long v;
            switch (kind) {
                case 0: v = rng() % 3; break;
                case 1: v = 5; break;
                case 2: v = (x + y) % 2; break;
                case 3: v = (x + y) % 3; break;
                case 4: v = y % 2 == 0 ? 1 : (y % 4 == 1 ? x == W - 1 : x == 0); break;          // a serpentine
                case 5: v = std::min(std::min(y, x), std::min(H - 1 - y, W - 1 - x)) % 3; break;
                default: v = (long long)(rng() % 4) - 1; break;                                 // with dead pixels
            }
            m.v[(size_t)y * W + x] = v;
        }
    return m;
}

int main() {
    // the key: larger size first, then the lower root; 0 is none
    if (!(rg_key(3, 10) > rg_key(2, 0) && rg_key(3, 4) > rg_key(3, 5) && rg_key(1, 0x7ffffffe) > 0 && rg_key_root(rg_key(7, 123456)) == 123456 &&
          rg_key_size(rg_key(0x7fffffff, 1)) == 0x7fffffff)) {
        std::printf("key order wrong\n");
        return 1;
    }
    if (!(rg_eligible(5, 4, 1, 1, 1, 1) && rg_eligible(5, 4, 0, 2, 0, 2) && !rg_eligible(5, 4, 0, 3, 1, 1) && !rg_eligible(15, 4, 1, 1, 1, 1) &&
          rg_eligible(0, 4, 0, 1, 0, 1) && !rg_eligible(0, 4, 0, 0, 2, 2))) {
        std::printf("eligibility wrong\n");
        return 1;
    }
    const int shapes[][2] = {{1, 1}, {1, 70}, {70, 1}, {7, 9}, {15, 17}, {16, 16}, {17, 15}, {33, 65}, {1, 4100}, {130, 150}};
    int cases = 0;
    for (auto& s : shapes)
        for (int kind = 0; kind < 7; ++kind)
            for (int conn = 4; conn <= 8; conn += 4)
                for (unsigned seed = 0; seed < 2; ++seed) {
                    const Map m = make(s[0], s[1], kind, 17 * seed + kind);
                    const int rc = run(m, conn, 1000 * seed + kind, seed == 0 ? 1 : 4);
                    if (rc) {
                        std::printf("FAILED %d x %d kind %d connectivity %d seed %u: %d\n", s[0], s[1], kind, conn, seed, rc);
                        return 1;
                    }
                    ++cases;
                }
    std::printf("ok: %d cases\n", cases);
    return 0;
}
