// A stand-alone host program over maskedsst_amd/csrc/msst_gmm_core.h: the Cholesky factorisation and the triangular inverse that
// msst_gmm_update runs in LDS, run here on the CPU as a team of one.  This is where a sanitizer belongs:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined tools/gmm_core_check.cpp -o gmm_core_check && ./gmm_core_check
// It is not part of the test suite.  Exit status 0 and "ok" when every case agrees.
//   1. S[i][j] = 1 / (1 + |i - j|) + (i == j) (1 + i / 4), 8 x 8, against numpy.linalg.cholesky, slogdet and inv written below;
//   2. a 96 x 96 covariance of condition number 1e6 in the kernel's pitch of 97 (heap arrays of exactly the size used, so that a
//      read or write past a row shows): L L^T = S, A L = I, and logdet against the known spectrum;
//   3. pivots that are zero, negative, NaN and infinite are refused, and nothing above the diagonal or in the pitch gap is touched.
#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>

#include "../maskedsst_amd/csrc/msst_gmm_core.h"

using namespace msst;

static const double NP_L[8][8] = {
    {1.4142135623730951, 0, 0, 0, 0, 0, 0, 0},
    {0.35355339059327373, 1.4577379737113252, 0, 0, 0, 0, 0, 0},
    {0.23570226039551581, 0.28583097523751472, 1.5371223432242522, 0, 0, 0, 0, 0},
    {0.17677669529663687, 0.18579013390438454, 0.2636281750481429, 1.6170133615603108, 0, 0, 0, 0},
    {0.1414213562373095, 0.13719886811400706, 0.16965748684549839, 0.25032774614221276, 1.6940273986145751, 0, 0, 0},
    {0.11785113019775791, 0.10861577059025559, 0.12437296967997062, 0.16050086448601059, 0.24034602259321544, 1.7678569941672448, 0, 0},
    {0.10101525445522105, 0.089832592217504628, 0.09791903644645307, 0.11727709580701873, 0.15392447641848514, 0.23211227543961971,
     1.8386993000468665, 0},
    {0.088388347648318433, 0.076561868367191435, 0.080637419902398533, 0.092078561571660944, 0.11231532481843873, 0.14865370643289944,
     0.22499959895331259, 1.9068317831334889},
};
static const double NP_LOGDET = 7.9706615452752585;
static const double NP_A_LAST[8] = {-0.014744380597796369, -0.013487399496338192, -0.014819493908663269, -0.017971361460311853,
                                    -0.023877999684142698, -0.035671958907732539, -0.064173932200864758, 0.52443010906641385};

static const double MARK = -12345.0;   // what the entries that must not be touched hold
static auto nosync = [] {};

static int small_case() {
    const int n = 8, p = 9;
    std::vector<double> a(n * p, MARK), row(n);
    for (int i = 0; i < n; ++i)
        for (int j = 0; j <= i; ++j) a[i * p + j] = 1.0 / (1.0 + (i - j)) + (i == j ? 1.0 + 0.25 * i : 0.0);
    double ld = 0.0;
    if (!gmm_cholesky(a.data(), n, p, 0, 1, nosync, &ld)) return 1;
    for (int i = 0; i < n; ++i)
        for (int j = 0; j <= i; ++j)
            if (std::fabs(a[i * p + j] - NP_L[i][j]) > 4e-16 * (1.0 + std::fabs(NP_L[i][j]))) return 2;
    if (std::fabs(ld - NP_LOGDET) > 1e-14) return 3;
    gmm_tri_inverse(a.data(), n, p, row.data(), 0, 1, nosync);
    for (int j = 0; j < n; ++j)
        if (std::fabs(a[(n - 1) * p + j] - NP_A_LAST[j]) > 1e-15) return 4;
    for (int i = 0; i < n; ++i)
        for (int j = i + 1; j < p; ++j)
            if (a[i * p + j] != MARK) return 5;
    return 0;
}

static int large_case() {
    const int n = 96, p = 97;
    // S = Q D Q^T with Q a product of Householder reflections and D log-spaced over six decades
    std::vector<double> q(n * n, 0.0), d(n), s(n * n, 0.0);
    for (int i = 0; i < n; ++i) q[i * n + i] = 1.0;
    unsigned state = 12345u;
    auto rnd = [&] { state = state * 1664525u + 1013904223u; return (double)(state >> 8) / 16777216.0 - 0.5; };
    for (int h = 0; h < 6; ++h) {
        std::vector<double> v(n);
        double nv = 0.0;
        for (int i = 0; i < n; ++i) { v[i] = rnd(); nv += v[i] * v[i]; }
        for (int r = 0; r < n; ++r) {
            double dot = 0.0;
            for (int i = 0; i < n; ++i) dot += q[r * n + i] * v[i];
            for (int i = 0; i < n; ++i) q[r * n + i] -= 2.0 * dot * v[i] / nv;
        }
    }
    double want_ld = 0.0;
    for (int i = 0; i < n; ++i) { d[i] = std::pow(10.0, -6.0 * i / (n - 1)); want_ld += std::log(d[i]); }
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j)
            for (int k = 0; k < n; ++k) s[i * n + j] += q[i * n + k] * d[k] * q[j * n + k];
    std::vector<double> a(n * p, MARK), row(n);
    for (int i = 0; i < n; ++i)
        for (int j = 0; j <= i; ++j) a[i * p + j] = 0.5 * (s[i * n + j] + s[j * n + i]);
    double ld = 0.0;
    if (!gmm_cholesky(a.data(), n, p, 0, 1, nosync, &ld)) return 1;
    if (std::fabs(ld - want_ld) > 1e-8) return 2;
    std::vector<double> l(a);
    double worst = 0.0;
    for (int i = 0; i < n; ++i)
        for (int j = 0; j <= i; ++j) {
            double v = 0.0;
            for (int k = 0; k <= j; ++k) v += l[i * p + k] * l[j * p + k];
            worst = std::fmax(worst, std::fabs(v - 0.5 * (s[i * n + j] + s[j * n + i])));
        }
    if (worst > 1e-14) return 3;
    gmm_tri_inverse(a.data(), n, p, row.data(), 0, 1, nosync);
    worst = 0.0;
    for (int i = 0; i < n; ++i)
        for (int j = 0; j <= i; ++j) {
            double v = 0.0;
            for (int k = j; k <= i; ++k) v += a[i * p + k] * l[k * p + j];
            worst = std::fmax(worst, std::fabs(v - (i == j ? 1.0 : 0.0)));
        }
    if (worst > 1e-9) return 4;   // condition number 1e3 of L against 2e-16
    for (int i = 0; i < n; ++i)
        for (int j = i + 1; j < p; ++j)
            if (a[i * p + j] != MARK) return 5;
    return 0;
}

static int refused_case() {
    const double bad[] = {0.0, -1.0, std::numeric_limits<double>::quiet_NaN(), std::numeric_limits<double>::infinity()};
    for (double b : bad)
        for (int at : {0, 3, 7}) {
            const int n = 8, p = 8;
            std::vector<double> a(n * p, MARK);
            for (int i = 0; i < n; ++i)
                for (int j = 0; j <= i; ++j) a[i * p + j] = i == j ? 2.0 : 0.0;
            a[at * p + at] = b;
            double ld = 0.0;
            if (gmm_cholesky(a.data(), n, p, 0, 1, nosync, &ld)) return 1;
            for (int i = 0; i < n; ++i)
                for (int j = i + 1; j < p; ++j)
                    if (a[i * p + j] != MARK) return 2;
        }
    return 0;
}

int main() {
    if (int rc = small_case()) { std::printf("FAILED against numpy, 8 x 8: %d\n", rc); return 1; }
    if (int rc = large_case()) { std::printf("FAILED 96 x 96: %d\n", rc); return 1; }
    if (int rc = refused_case()) { std::printf("FAILED refused pivots: %d\n", rc); return 1; }
    std::printf("ok\n");
    return 0;
}
