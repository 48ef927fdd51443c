// Stand-alone check of trep_amd/csrc/sym_eig.hpp on the host (TEAM = 1), for a run under a host sanitizer:
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -o sym_eig_main sym_eig_main.cpp && ./sym_eig_main
// Symmetric matrices of every order 0 .. 17 (odd and even: the dummy index of the round-robin ordering) in images of the kernel's
// leading dimension, allocated to the word so that an access outside an image is an error; the answer is checked against
// A = Y diag(lambda) Y' and Y'Y = I.  Exit status 0: every order within 1e-12.  TEST INFRASTRUCTURE ONLY.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../trep_amd/csrc/sym_eig.hpp"

int main() {
    unsigned long long seed = 88172645463325252ull;
    auto rnd = [&]() { seed ^= seed << 13; seed ^= seed >> 7; seed ^= seed << 17; return (double)(seed >> 11) / (double)(1ull << 53) - 0.5; };
    double worst = 0.0;
    for (int n = 0; n <= 17; n++) for (int n_trips = n; n_trips <= n + 2; n_trips++) {
        const int ld = tg::sym_eig_ld(n_trips);
        std::vector<double> A((size_t)n * ld), Y((size_t)n * ld), A0, cs((size_t)tg::sym_eig_scratch_doubles(n_trips));
        for (int i = 0; i < n; i++) for (int j = 0; j <= i; j++) { const double v = rnd() * (i % 3 == 0 ? 100.0 : 1.0); A[i * ld + j] = v; A[j * ld + i] = v; }
        for (int i = 0; i < n; i++) for (int j = 0; j < n; j++) Y[i * ld + j] = i == j ? 1.0 : 0.0;
        A0 = A;
        bool converged = false;
        const int sweeps = tg::sym_eig_jacobi<1>(true, A.data(), Y.data(), n, n_trips, ld, 30, cs.data(), 0, converged, [](bool f) { return f; });
        if (!converged) { std::printf("order %d: not converged after %d sweeps\n", n, sweeps); return 1; }
        double scale = 1.0;
        for (int i = 0; i < n; i++) for (int j = 0; j < n; j++) if (std::fabs(A0[i * ld + j]) > scale) scale = std::fabs(A0[i * ld + j]);
        for (int i = 0; i < n; i++) for (int j = 0; j < n; j++) {
            double rec = 0.0, dot = 0.0;
            for (int k = 0; k < n; k++) { rec += Y[i * ld + k] * A[k * ld + k] * Y[j * ld + k]; dot += Y[k * ld + i] * Y[k * ld + j]; }
            const double e1 = std::fabs(rec - A0[i * ld + j]) / scale, e2 = std::fabs(dot - (i == j ? 1.0 : 0.0));
            if (e1 > worst) worst = e1;
            if (e2 > worst) worst = e2;
        }
    }
    std::printf("worst error %.3e\n", worst);
    return worst <= 1e-12 ? 0 : 1;
}
