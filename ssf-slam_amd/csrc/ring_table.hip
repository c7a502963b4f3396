// ring_table.hip -- host: the ring-id table (RingTable, feat_common.hpp) that every feature
// kernel looks a point's row up in.  build_ring_table evaluates the reference's exact chain
// (frameFeature.cpp:57-73) with the host libm -- the float overloads or the all-double chain, as
// oracle/ssf_oracle.c -- finds every ratio at which the row id changes, and cuts the ratio axis
// into kRingCells cells of at most two ids each.  No device code of its own.
#include "feat_common.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

namespace ssf {

namespace {
constexpr double kPi = 3.14159265358979323846;       // M_PI
// the bin arithmetic of a float angle (frameFeature.cpp:58-73; oracle/ssf_oracle.c orc_ring_id_of_angle)
int angle_id(float angle, int n_rows) {
    if (angle != angle) return -1;
    int id = -1;
    if (n_rows == 16) {
        const double v = (double)((angle + 15.0f) / 2.0f) + 0.5;
        id = v > -2147483648.0 && v < 2147483647.0 ? (int)v : -1;
    } else if (n_rows == 64) {
        const double v = (double)angle >= -8.83 ? (double)(2.0f - angle) * 3.0 + 0.5 : (-8.83 - (double)angle) * 2.0 + 0.5;
        const int t = v > -2147483648.0 && v < 2147483647.0 ? (int)v : -1000;
        id = (double)angle >= -8.83 ? t : (t == -1000 ? -1 : n_rows / 2 + t);
    }
    return (id > -1 && id < n_rows) ? id : -1;
}
// the float chain's id of its float ratio: atanf, `* 180` in float, `/ M_PI` in double, to float
int id_float_chain(float ratio, int n_rows) {
    if (ratio != ratio) return -1;
    const float deg = ::atanf(ratio) * 180.0f;
    return angle_id((float)((double)deg / kPi), n_rows);
}
// the double chain's id of its double ratio
int id_double_chain(double ratio, int n_rows) {
    if (ratio != ratio) return -1;
    return angle_id((float)(::atan(ratio) * 180.0 / kPi), n_rows);
}
uint32_t fkey(float f) { uint32_t b; std::memcpy(&b, &f, 4); return (b & 0x80000000u) ? ~b : (b | 0x80000000u); }
float kfloat(uint32_t k) { const uint32_t b = (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k; float f; std::memcpy(&f, &b, 4); return f; }
uint64_t dkey(double d) { uint64_t b; std::memcpy(&b, &d, 8); return (b >> 63) ? ~b : (b | (1ull << 63)); }
double kdouble(uint64_t k) { const uint64_t b = (k >> 63) ? (k & ~(1ull << 63)) : ~k; double d; std::memcpy(&d, &b, 8); return d; }
int host_cell(float ratio, float r0, float inv) {   // the device's cell, the same float ops
    const float tc = (ratio - r0) * inv;
    return tc < 0.0f ? 0 : (tc >= (float)kRingCells ? kRingCells - 1 : std::min((int)tc, kRingCells - 1));
}
// smallest key in [lo, hi] with pred true (pred monotone false -> true on the range; hi must satisfy it)
template <class K, class P> K first_key(K lo, K hi, P pred) {
    while (lo < hi) {
        const K m = lo + (hi - lo) / 2;
        if (pred(m)) hi = m; else lo = m + 1;
    }
    return lo;
}
}  // namespace

int build_ring_table(int n_rows, int chain, void* out_host) {
    if (chain != kRingChainFloat && chain != kRingChainDouble) return -5;
    const bool dbl = chain == kRingChainDouble;
    RingTable& T = *reinterpret_cast<RingTable*>(out_host);
    std::memset(&T, 0, sizeof(T));
    T.chain = chain;
    if (n_rows == 64) { T.r0 = -0.5f; T.inv = (float)kRingCells / 0.6f; }
    else { T.r0 = -0.4f; T.inv = (float)kRingCells / 0.8f; }
    // the id of a ratio given as a double (the float chain's ratios are floats: exact in double)
    auto id_of = [&](double r) { return dbl ? id_double_chain(r, n_rows) : id_float_chain((float)r, n_rows); };
    if (id_of(-INFINITY) != id_of(-2.0) || id_of(INFINITY) != id_of(2.0)) return -1;
    // the id's change points: brackets from a dense sweep of [-2, 2] (the ids are -1 beyond),
    // each refined to the exact first ratio of the new id (first float / first double)
    std::vector<double> chg;
    double prev_r = -2.0;
    int prev_id = id_of(prev_r);
    for (int k = 1; k <= 40000; ++k) {
        const double r = (double)(-2.0f + 4.0f * (float)k / 40000.0f);
        const int id = id_of(r);
        if (id != prev_id) {
            const int a = prev_id;
            if (dbl) chg.push_back(kdouble(first_key<uint64_t>(dkey(prev_r) + 1, dkey(r), [&](uint64_t q) { return id_of(kdouble(q)) != a; })));
            else chg.push_back(kfloat(first_key<uint32_t>(fkey((float)prev_r) + 1, fkey((float)r), [&](uint32_t q) { return id_of(kfloat(q)) != a; })));
            if (id_of(chg.back()) != id) return -2;                           // two changes in one bracket
        }
        prev_r = r; prev_id = id;
    }
    int seen[kMaxRows] = {};
    for (int r = 0; r < kMaxRows; ++r) { T.rlo[r] = INFINITY; T.rhi[r] = -INFINITY; }
    for (size_t i = 0; i + 1 < chg.size(); ++i) {             // the constant-id intervals between changes
        const int id = id_of(chg[i]);
        if (id < 0 || id >= kMaxRows) continue;
        if (++seen[id] == 1) { T.rlo[id] = (float)chg[i]; T.rhi[id] = (float)chg[i + 1]; }
        else { T.rlo[id] = INFINITY; T.rhi[id] = -INFINITY; }   // a split row: never regular
    }
    const uint32_t kmin = fkey(-INFINITY), kmax = fkey(INFINITY);
    for (int c = 0; c < kRingCells; ++c) {
        // the cell's floats [ks, ke]; a change point T belongs to the cell of its float rounding
        // (the device looks a double ratio up in the cell of its float rounding; a float chain
        // ratio is its own rounding)
        const uint32_t ks = c == 0 ? kmin : first_key<uint32_t>(kmin, kmax, [&](uint32_t q) { return host_cell(kfloat(q), T.r0, T.inv) >= c; });
        if (c > 0 && host_cell(kfloat(ks), T.r0, T.inv) != c) return -3;   // an empty cell
        int nchg = 0;
        double at = 0.0;
        for (double q : chg) if (host_cell((float)q, T.r0, T.inv) == c) { ++nchg; at = q; }
        if (nchg > 1) return -4;                                             // cells too wide
        // below the change (or the whole cell): the id of the cell's first float
        const int a = nchg ? id_of(dbl ? kdouble(dkey(at) - 1) : (double)kfloat(fkey((float)at) - 1))
                           : id_of((double)kfloat(ks));
        const int b = nchg ? id_of(at) : a;
        T.cell[c].thr = nchg ? (float)at : INFINITY;
        T.dthr[c] = nchg ? at : INFINITY;
        T.cell[c].ids = (int32_t)(((uint32_t)(uint8_t)(int8_t)a) | ((uint32_t)(uint8_t)(int8_t)b << 8));
    }
    return 0;
}
size_t ring_table_bytes() { return sizeof(RingTable); }

}  // namespace ssf
