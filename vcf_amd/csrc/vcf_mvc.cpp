// vcf_mvc.cpp -- the coded motion field of the IPP coder (--mvc, not in the
// reference): median prediction from the neighbours and signed exp-Golomb codes
// of order 0; vcf_mv_encode, vcf_mv_decode and vcf_mv_encode_bound of the C
// ABI.  Native host code beside the other entropy coders.  The rule is stated
// in include/vcf_amd.h ("Coded motion fields") and restated in plain Python by
// tests/mvc_ref.py; vcf_mvc.h holds the predictor and the code length, which the
// refinement kernel (vcf_ipp_mvrefine.hip) shares.
//
// A stream is the codes of dx then dy of every block in raster order, MSB
// first, the last byte padded with zero bits.  The decoder checks every read
// against the stream's end, so a corrupt stream ends in VCF_ERR_INVALID and
// never in a read or a write out of bounds.
#include <cstdint>

#include "vcf_amd.h"
#include "vcf_internal.h"
#include "vcf_mvc.h"

namespace vcf {
namespace {

constexpr int kMaxQ = 1 << 15;          // |q| of a coded vector, in quarter pels
constexpr int kMaxPrefix = 17;          // |d| <= 2^16 -> k + 1 <= 2^17 + 1
constexpr int kMaxBlockBits = 2 * (2 * kMaxPrefix + 1);
constexpr int64_t kMaxBlocks = (int64_t)1 << 40;

bool bad_step(int32_t step) { return step != 1 && step != 2 && step != 4; }

int check_field(int32_t nby, int32_t nbx, int32_t step)
{
    if (nby < 0 || nbx < 0 || (int64_t)nby * nbx > kMaxBlocks)
        return set_error(VCF_ERR_INVALID, "motion field of %d x %d blocks", nby, nbx);
    if (bad_step(step)) return set_error(VCF_ERR_INVALID, "vector step %d (1, 2 or 4 quarter pels)", step);
    return VCF_OK;
}

struct BitWriter {
    uint8_t *out;
    int64_t cap, n = 0;   // n: whole bytes written
    uint32_t acc = 0;     // the pending bits, right-aligned
    int fill = 0;

    bool put(uint32_t v, int bits)   // the low `bits` of v, MSB first; bits <= 18
    {
        acc = (acc << bits) | v;
        fill += bits;
        while (fill >= 8) {
            if (n >= cap) return false;
            out[n++] = (uint8_t)(acc >> (fill - 8));
            fill -= 8;
        }
        acc &= (1u << fill) - 1;
        return true;
    }
    bool flush() { return fill == 0 || put(0, 8 - fill); }
};

struct BitReader {
    const uint8_t *in;
    int64_t nbits, pos = 0;

    int bit()   // -1 past the end
    {
        if (pos >= nbits) return -1;
        const int b = (in[pos >> 3] >> (7 - (int)(pos & 7))) & 1;
        ++pos;
        return b;
    }
};

// one signed exp-Golomb code: z zeros, then k + 1 in z + 1 bits
bool put_code(BitWriter &w, int32_t d)
{
    const uint32_t v = mv_code_index(d) + 1;
    const int z = 31 - __builtin_clz(v);
    return w.put(0, z) && w.put(v, z + 1);
}

int get_code(BitReader &r, int32_t *d)
{
    int z = 0, b;
    while ((b = r.bit()) == 0)
        if (++z > kMaxPrefix) return set_error(VCF_ERR_INVALID, "motion stream: a prefix of more than %d zeros", kMaxPrefix);
    if (b < 0) return set_error(VCF_ERR_INVALID, "motion stream ends inside a code");
    uint32_t v = 1;
    for (int i = 0; i < z; ++i) {
        if ((b = r.bit()) < 0) return set_error(VCF_ERR_INVALID, "motion stream ends inside a code");
        v = (v << 1) | (uint32_t)b;
    }
    const uint32_t k = v - 1;
    *d = (k & 1) ? (int32_t)((k + 1) >> 1) : -(int32_t)(k >> 1);
    return VCF_OK;
}

}  // namespace
}  // namespace vcf

using namespace vcf;

extern "C" {

int vcf_mv_encode_bound(int32_t nby, int32_t nbx, int64_t *bytes)
{
    if (!bytes) return set_error(VCF_ERR_INVALID, "null pointer");
    const int rc = check_field(nby, nbx, 1);
    if (rc != VCF_OK) return rc;
    *bytes = ((int64_t)nby * nbx * kMaxBlockBits + 7) / 8;
    return VCF_OK;
}

int vcf_mv_encode(const int32_t *q, int32_t nby, int32_t nbx, int32_t step, uint8_t *out, int64_t cap, int64_t *nbytes)
{
    if (!q || !out || !nbytes) return set_error(VCF_ERR_INVALID, "null pointer");
    const int rc = check_field(nby, nbx, step);
    if (rc != VCF_OK) return rc;
    if (cap < 0) return set_error(VCF_ERR_INVALID, "capacity %lld", (long long)cap);
    const int64_t n = (int64_t)nby * nbx;
    for (int64_t t = 0; t < 2 * n; ++t) {
        if (q[t] > kMaxQ || q[t] < -kMaxQ)
            return set_error(VCF_ERR_INVALID, "vector component %d quarter pels (within +-%d)", q[t], kMaxQ);
        if (q[t] % step != 0) return set_error(VCF_ERR_INVALID, "vector component %d is no multiple of the step %d", q[t], step);
    }
    BitWriter w{out, cap};
    for (int by = 0; by < nby; ++by)
        for (int bx = 0; bx < nbx; ++bx) {
            const MvQ p = mv_predictor(q, nbx, by, bx);
            const int32_t *v = q + ((int64_t)by * nbx + bx) * 2;
            if (!put_code(w, (v[0] - p.x) / step) || !put_code(w, (v[1] - p.y) / step))
                return set_error(VCF_ERR_INVALID, "capacity %lld below the stream (vcf_mv_encode_bound)", (long long)cap);
        }
    if (!w.flush()) return set_error(VCF_ERR_INVALID, "capacity %lld below the stream (vcf_mv_encode_bound)", (long long)cap);
    *nbytes = w.n;
    return VCF_OK;
}

int vcf_mv_decode(const uint8_t *in, int64_t nbytes, int32_t nby, int32_t nbx, int32_t step, int32_t *q)
{
    if (!in || !q) return set_error(VCF_ERR_INVALID, "null pointer");
    int rc = check_field(nby, nbx, step);
    if (rc != VCF_OK) return rc;
    if (nbytes < 0 || nbytes > (int64_t)1 << 59) return set_error(VCF_ERR_INVALID, "stream of %lld bytes", (long long)nbytes);
    BitReader r{in, nbytes * 8};
    for (int by = 0; by < nby; ++by)
        for (int bx = 0; bx < nbx; ++bx) {
            const MvQ p = mv_predictor(q, nbx, by, bx);   // reads decoded vectors only
            int32_t d[2];
            for (int c = 0; c < 2; ++c)
                if ((rc = get_code(r, &d[c])) != VCF_OK) return rc;
            // |p| <= 2^15 and |d| <= 2^17: no overflow
            const int32_t x = p.x + d[0] * step, y = p.y + d[1] * step;
            if (x > kMaxQ || x < -kMaxQ || y > kMaxQ || y < -kMaxQ)
                return set_error(VCF_ERR_INVALID, "motion stream: vector (%d, %d) quarter pels (within +-%d)", x, y, kMaxQ);
            int32_t *v = q + ((int64_t)by * nbx + bx) * 2;
            v[0] = x;
            v[1] = y;
        }
    if ((r.pos + 7) / 8 != nbytes) return set_error(VCF_ERR_INVALID, "motion stream: bytes after the last code");
    int b;
    while ((b = r.bit()) >= 0)
        if (b) return set_error(VCF_ERR_INVALID, "motion stream: padding bits set");
    return VCF_OK;
}

}  // extern "C"
