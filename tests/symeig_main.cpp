// Stand-alone check of csrc/symeig.h (the projected eigenproblem of dcfm_sigma_eigs), built by
// tests/test_symeig_host.py with the host compiler and -fsanitize=address,undefined.
// For every matrix: max |A V - V D| <= 64 n eps ||A||_max-row-sum and max |V'V - I| <= 64 n eps,
// eigenvalues ascending; known spectra are compared as well.  Exit status 0 = all passed.
#include "symeig.h"

#include <cstdio>
#include <cstdlib>
#include <vector>

static const double EPS = 2.220446049250313e-16;
static int failures = 0;

static double norm_inf(const std::vector<double> &A, int n) {
    double m = 0.0;
    for (int i = 0; i < n; ++i) {
        double s = 0.0;
        for (int j = 0; j < n; ++j) s += std::fabs(A[(size_t)i * n + j]);
        m = std::max(m, s);
    }
    return m;
}

// residual and orthonormality of symeig(A); expect (nullable): the ascending spectrum
static void check(const char *name, const std::vector<double> &A, int n, const double *expect) {
    std::vector<double> w, V;
    const bool ok = dcfm::symeig(A.data(), n, w, V);
    const double na = std::max(norm_inf(A, n), 1e-300), bound = 64.0 * n * EPS;
    double res = 0.0, orth = 0.0, spec = 0.0;
    bool sorted = true;
    for (int j = 0; j < n; ++j) {
        if (j && w[j] < w[j - 1]) sorted = false;
        for (int i = 0; i < n; ++i) {
            double av = 0.0, vv = 0.0;
            for (int k = 0; k < n; ++k) {
                av += A[(size_t)i * n + k] * V[(size_t)k * n + j];
                vv += V[(size_t)k * n + i] * V[(size_t)k * n + j];
            }
            res = std::max(res, std::fabs(av - V[(size_t)i * n + j] * w[j]));
            orth = std::max(orth, std::fabs(vv - (i == j ? 1.0 : 0.0)));
        }
        if (expect) spec = std::max(spec, std::fabs(w[j] - expect[j]));
    }
    const bool pass = ok && sorted && res <= bound * na && orth <= bound && spec <= bound * na;
    std::printf("%-12s n=%3d  resid %.3e (<= %.3e)  orth %.3e (<= %.3e)  spectrum %.3e  %s\n", name, n, res,
                bound * na, orth, bound, spec, pass ? "ok" : "FAIL");
    if (!pass) ++failures;
}

int main() {
    {   // diagonal, unsorted, with a negative entry
        const int n = 5;
        const double dg[n] = {3.0, -1.0, 7.5, 0.0, 2.0}, ex[n] = {-1.0, 0.0, 2.0, 3.0, 7.5};
        std::vector<double> A(n * n, 0.0);
        for (int i = 0; i < n; ++i) A[i * n + i] = dg[i];
        check("diagonal", A, n, ex);
    }
    {   // [[2, 1], [1, 2]]: eigenvalues 1 and 3
        const std::vector<double> A = {2.0, 1.0, 1.0, 2.0};
        const double ex[2] = {1.0, 3.0};
        check("2x2", A, 2, ex);
    }
    {   // 1 x 1
        const std::vector<double> A = {-4.25};
        const double ex[1] = {-4.25};
        check("1x1", A, 1, ex);
    }
    {   // 64 x 64: Q D Q' with Q a product of three Householder reflections, a repeated eigenvalue
        const int n = 64;
        std::vector<double> D(n), A((size_t)n * n, 0.0);
        for (int i = 0; i < n; ++i) D[i] = (i < 8) ? 2.0 : 0.25 * (i - 20);   // 2.0 eight times (and once more at i = 28)
        for (int i = 0; i < n; ++i) A[(size_t)i * n + i] = D[i];
        unsigned long long st = 12345;
        for (int rep = 0; rep < 3; ++rep) {
            std::vector<double> u(n);
            double nu = 0.0;
            for (int i = 0; i < n; ++i) {
                st = st * 6364136223846793005ull + 1442695040888963407ull;
                u[i] = (double)(st >> 11) * 0x1.0p-53 - 0.5;
                nu += u[i] * u[i];
            }
            for (int i = 0; i < n; ++i) u[i] /= std::sqrt(nu);
            // A <- H A H, H = I - 2 u u'
            std::vector<double> Au(n, 0.0);
            for (int i = 0; i < n; ++i)
                for (int k = 0; k < n; ++k) Au[i] += A[(size_t)i * n + k] * u[k];
            double uAu = 0.0;
            for (int i = 0; i < n; ++i) uAu += u[i] * Au[i];
            for (int i = 0; i < n; ++i)
                for (int j = 0; j < n; ++j)
                    A[(size_t)i * n + j] += -2.0 * u[i] * Au[j] - 2.0 * Au[i] * u[j] + 4.0 * uAu * u[i] * u[j];
        }
        for (int i = 0; i < n; ++i)   // exactly symmetric input
            for (int j = 0; j < i; ++j) A[(size_t)i * n + j] = A[(size_t)j * n + i];
        std::sort(D.begin(), D.end());
        check("householder", A, n, D.data());
    }
    if (failures) std::printf("%d case(s) failed\n", failures);
    return failures ? 1 : 0;
}
