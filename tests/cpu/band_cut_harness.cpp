// vcf_band_cut.h (the band cut of the 2D-DWT launchers, host only) behind a C
// entry point for tests/test_dwt_schedule.py.
#include "vcf_band_cut.h"

extern "C" int bc_band_cut(int rows, int max_bands, long long per_band, long long slots, int steps_per_row,
                           int overhead)
{
    return vcf::band_cut(rows, max_bands, per_band, slots, steps_per_row, overhead);
}
