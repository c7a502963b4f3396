// numpy_rng.hpp -- the host RandomState of the GMM k-means++ init: MT19937 with numpy's legacy
// seeding, random_sample and choice(n, p=ones/n).  Host arithmetic only, nothing from HIP.
#pragma once
#include <algorithm>
#include <cstdint>
#include <map>
#include <vector>

namespace ssf {

struct NumpyRandomState {
    uint32_t mt[624];
    int mt_pos = 625;                                   // 625: never seeded (5489 on first use)
    std::map<int64_t, std::vector<double>> cdf_cache;   // choice(n, p=1/n) cumulative table

    void seed(uint32_t s) {
        mt[0] = s;
        for (int i = 1; i < 624; ++i) mt[i] = 1812433253u * (mt[i - 1] ^ (mt[i - 1] >> 30)) + (uint32_t)i;
        mt_pos = 624;
    }

    uint32_t next_u32() {
        if (mt_pos >= 624) {
            if (mt_pos > 624) seed(5489u);
            for (int i = 0; i < 624; ++i) {
                uint32_t y = (mt[i] & 0x80000000u) | (mt[(i + 1) % 624] & 0x7fffffffu);
                mt[i] = mt[(i + 397) % 624] ^ (y >> 1) ^ ((y & 1u) ? 0x9908b0dfu : 0u);
            }
            mt_pos = 0;
        }
        uint32_t y = mt[mt_pos++];
        y ^= (y >> 11);
        y ^= (y << 7) & 0x9d2c5680u;
        y ^= (y << 15) & 0xefc60000u;
        y ^= (y >> 18);
        return y;
    }

    double random_sample() {
        uint32_t a = next_u32() >> 5, b = next_u32() >> 6;
        return ((double)a * 67108864.0 + (double)b) / 9007199254740992.0;
    }

    // numpy RandomState.choice(n, p=ones/n): cdf = cumsum(p); cdf /= cdf[-1];
    // searchsorted(cdf, u, side='right')  (sklearn _kmeans_plusplus first centre).
    int64_t choice_uniform(int64_t n, double u) {
        auto it = cdf_cache.find(n);
        if (it == cdf_cache.end()) {
            if (cdf_cache.size() > 8) cdf_cache.clear();
            std::vector<double> cdf((size_t)n);
            const double p = 1.0 / (double)n;
            double s = 0.0;
            for (int64_t i = 0; i < n; ++i) { s += p; cdf[(size_t)i] = s; }
            const double last = cdf[(size_t)n - 1];
            for (auto& v : cdf) v /= last;
            it = cdf_cache.emplace(n, std::move(cdf)).first;
        }
        const auto& cdf = it->second;
        auto pos = std::upper_bound(cdf.begin(), cdf.end(), u);
        int64_t idx = (int64_t)(pos - cdf.begin());
        return idx < n ? idx : n - 1;
    }
};

}  // namespace ssf
