// Host build of the encode's provable-zero row test (vcf_amd/csrc/vcf_dct_block.h:
// row_abs_sum, row_pair_is_zero) next to the real row pass it stands in for,
// for tests/test_block_math_skip.py.
#include <string.h>

#include "vcf_dct_block.h"

using namespace vcf;

static float qd0_of(int Q)
{
    return (float)(1.0 / ((double)Q * 8.0));   // make_enc_consts: qd[0] of a power-of-two Q
}

// n row pairs (rows ua[k], ub[k] of 8 floats in the column pass's units):
// skip[k] = the test's verdict, idx[k][0..15] = the indices the row pass gives
extern "C" void hs_row_pairs(int n, const float *ua, const float *ub, int Q, uint8_t *skip, int32_t *idx)
{
    const float kb = row_skip_scale(qd0_of(Q));
    const FinalK rowk = row_final_k(Q);
    for (int k = 0; k < n; ++k) {
        const float *a = ua + 8 * k, *b = ub + 8 * k;
        const float sa = row_abs_sum(a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[7]);
        const float sb = row_abs_sum(b[0], b[1], b[2], b[3], b[4], b[5], b[6], b[7]);
        skip[k] = row_pair_is_zero(sa, sb, kb) ? 1 : 0;
        float ra[8], rb[8];
        memcpy(ra, a, sizeof ra);
        memcpy(rb, b, sizeof rb);
        dct2_8f(ra, rowk);
        dct2_8f(rb, rowk);
        for (int j = 0; j < 8; ++j) {
            idx[16 * k + j] = cvt_trunc_i32(ra[j]);
            idx[16 * k + 8 + j] = cvt_trunc_i32(rb[j]);
        }
    }
}

template <int C>
static void colpass(const uint8_t *rgb, float (&v)[8][8])
{
    uint32_t raw[8][6];
    memcpy(raw, rgb, 192);
    constexpr float cs = C == 1 ? 0.5f : 0.25f;
    constexpr FinalK colk = final_k(cs * 0.25f, cs * 0.5f);
    float dep = 0.0f;
    fold_columns<C, 0, false>(raw, ycocg_magic_word<C>(), colk, v, dep);
}

// n blocks of 192 RGB bytes: v[k][c] = the 8x8 column-pass output of channel c
extern "C" void hs_colpass(int n, const uint8_t *rgb, float *v)
{
    for (int k = 0; k < n; ++k) {
        float(*o)[8][8] = reinterpret_cast<float(*)[8][8]>(v + (size_t)k * 192);
        colpass<0>(rgb + (size_t)k * 192, o[0]);
        colpass<1>(rgb + (size_t)k * 192, o[1]);
        colpass<2>(rgb + (size_t)k * 192, o[2]);
    }
}

// n blocks: pass[k][c][p - 1] = the verdict for row pair p = 1..3 of channel c
extern "C" void hs_block_verdicts(int n, const uint8_t *rgb, int Q, uint8_t *pass)
{
    const float kb = row_skip_scale(qd0_of(Q));
    for (int k = 0; k < n; ++k) {
        float v[3][8][8];
        colpass<0>(rgb + (size_t)k * 192, v[0]);
        colpass<1>(rgb + (size_t)k * 192, v[1]);
        colpass<2>(rgb + (size_t)k * 192, v[2]);
        for (int c = 0; c < 3; ++c)
            for (int p = 1; p < 4; ++p) {
                const float *a = v[c][2 * p], *b = v[c][2 * p + 1];
                const float sa = row_abs_sum(a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[7]);
                const float sb = row_abs_sum(b[0], b[1], b[2], b[3], b[4], b[5], b[6], b[7]);
                pass[(k * 3 + c) * 3 + p - 1] = row_pair_is_zero(sa, sb, kb) ? 1 : 0;
            }
    }
}
