// numpy_rng_main.cpp -- drives csrc/numpy_rng.hpp from the command line for
// tests/test_numpy_rng_host.py.  One NumpyRandomState, unseeded at start; commands on stdin, one
// per line, results on stdout, one per line:
//   seed S        seed(S)
//   sample N      N x random_sample(), %.17g
//   choice N U    choice_uniform(N, U)
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "numpy_rng.hpp"

int main() {
    ssf::NumpyRandomState rs;
    char cmd[16];
    while (std::scanf("%15s", cmd) == 1) {
        if (!std::strcmp(cmd, "seed")) {
            unsigned long long s;
            if (std::scanf("%llu", &s) != 1) return 2;
            rs.seed((uint32_t)s);
        } else if (!std::strcmp(cmd, "sample")) {
            long long n;
            if (std::scanf("%lld", &n) != 1) return 2;
            for (long long i = 0; i < n; ++i) std::printf("%.17g\n", rs.random_sample());
        } else if (!std::strcmp(cmd, "choice")) {
            long long n;
            char u[64];
            if (std::scanf("%lld %63s", &n, u) != 2 || n < 1) return 2;
            std::printf("%lld\n", (long long)rs.choice_uniform(n, std::strtod(u, nullptr)));
        } else {
            return 2;
        }
    }
    return 0;
}
