// vcf_band_cut.h -- the band cut of the 2D-DWT kernels that walk a plane in
// horizontal bands (host only; tests/test_dwt_schedule.py builds it with g++).
//
// A launch of n_bands x per_band workgroups runs in rounds of `slots` resident
// workgroups, and every workgroup takes steps_per_row steps per row of its
// band plus `overhead` steps of halo and pipeline warm-up, so
//   time ~ ceil(per_band * n_bands / slots) * (steps_per_row * band_rows + overhead).
// More bands shorten the bands but pay the overhead again and, past a full
// round, add a round.
#pragma once
#include <algorithm>

namespace vcf {

// The number of bands, 1 .. max_bands, that minimises the model's time for
// `rows` rows (the fewest bands on a tie); only cuts whose last band is not
// empty count.  Callers cut the plane into ceil(rows / n_bands)-row bands.
inline int band_cut(int rows, int max_bands, long long per_band, long long slots, int steps_per_row, int overhead)
{
    int n_bands = 1;
    long long best = -1;
    for (int nb = 1; nb <= std::max(1, max_bands); ++nb) {
        const int br = (rows + nb - 1) / nb;
        if (nb > 1 && (rows + br - 1) / br != nb) continue;
        const long long rounds = (per_band * nb + slots - 1) / slots;
        const long long cost = rounds * ((long long)steps_per_row * br + overhead);
        if (best < 0 || cost < best) {
            best = cost;
            n_bands = nb;
        }
    }
    return n_bands;
}

}  // namespace vcf
