// Host build of vcf_cbaac_coder.h (g++, no GPU): a whole-segment order-0 encoder and decoder made of the
// header's functions, with the plainest model (a 257-entry cumulative array, the reference's update and
// halving rule) and a byte-vector writer and reader.  tests/test_cbaac_coder.py compares its bytes with the
// serial coder's (vcf_cbaac_encode) and checks floordiv / floordiv_big against integer division.
#include <cstdint>
#include <cstring>
#include <vector>

#include "vcf_cbaac_coder.h"

using namespace vcf::a8;

namespace {

constexpr uint32_t kMaxFreq = 16384;   // AdaptiveModel(max_freq=16384)

struct Model {
    uint32_t c[257];   // c[s] = sum of freq[0..s), c[256] = total
    Model()
    {
        for (int s = 0; s <= 256; ++s) c[s] = (uint32_t)s;
    }
    void update(int s)   // freq[s] += 1; every freq -> (f >> 1) + 1 if the total before was >= max_freq
    {
        const uint32_t stale = c[256];
        for (int t = s + 1; t <= 256; ++t) ++c[t];
        if (stale < kMaxFreq) return;
        uint32_t run = 0;
        for (int t = 0; t < 256; ++t) {
            const uint32_t f = ((c[t + 1] - c[t]) >> 1) + 1;
            c[t] = run;
            run += f;
        }
        c[256] = run;
    }
};

struct VectorStore {
    std::vector<uint8_t> *out;
    void operator()(uint64_t i, uint32_t word) const   // `word` is byte-swapped: little-endian bytes are the stream's
    {
        if (out->size() < 4 * i + 4) out->resize(4 * i + 4);
        for (int k = 0; k < 4; ++k) (*out)[4 * i + k] = (uint8_t)(word >> (8 * k));
    }
};
using Writer = BitWriter<uint64_t, VectorStore>;

// the header's encoder sink, counting what the test wants to have seen
struct CountingEmit {
    Emit<Writer, uint64_t> emit;
    int64_t *stats;   // [1] steps with d > 0, [2] steps with p > 0, [3] longest pending run written here
    void common(uint32_t top, uint32_t d)
    {
        ++stats[1];
        if ((int64_t)emit.pending > stats[3]) stats[3] = (int64_t)emit.pending;
        emit.common(top, d);
    }
    void underflow(uint32_t p)
    {
        ++stats[2];
        emit.underflow(p);
    }
};

struct Reader {   // MSB-first, zeros past the end
    const uint8_t *p;
    int64_t nbits, pos = 0;
    uint32_t get(uint32_t k)
    {
        uint32_t v = 0;
        for (uint32_t i = 0; i < k; ++i, ++pos) v = (v << 1) | (pos < nbits ? (p[pos >> 3] >> (7 - (pos & 7))) & 1u : 0u);
        return v;
    }
};

}  // namespace

extern "C" {

// sym[0..n) -> out (at most cap bytes are copied); returns the stream's size in bytes.
// stats[0..5): steps, steps with d > 0, steps with p > 0, the longest run of pending bits written by a
// renormalisation, the run written by the flush
int64_t cc_encode(const uint8_t *sym, int64_t n, uint8_t *out, int64_t cap, int64_t *stats)
{
    std::vector<uint8_t> buf;
    Writer w{{&buf}};
    Model m;
    uint32_t low = 0, high = 0xFFFFFFFFu;
    uint64_t pending = 0;
    for (int k = 0; k < 5; ++k) stats[k] = 0;
    for (int64_t i = 0; i < n; ++i) {
        const int s = sym[i];
        const double tot = (double)m.c[256];
        narrow(low, high, m.c[s], m.c[s + 1], tot, 1.0 / tot);
        renorm(low, high, CountingEmit{{w, pending}, stats});
        ++stats[0];
        m.update(s);
    }
    stats[4] = (int64_t)pending + 1;
    encode_flush(w, low, pending);
    const int64_t nbytes = (int64_t)((w.finish() + 7) / 8);
    buf.resize((size_t)nbytes);   // the last word's bytes past the last bit are not part of the stream
    if (nbytes) memcpy(out, buf.data(), (size_t)(nbytes < cap ? nbytes : cap));
    return nbytes;
}

// the lane decoder's search: scaled = floor(((T + 1) total - 1) / range) by floordiv_big, the symbol by a scan
void cc_decode(const uint8_t *in, int64_t nbytes, int64_t n, uint8_t *sym)
{
    Reader br{in, 8 * nbytes};
    Model m;
    uint32_t low = 0, high = 0xFFFFFFFFu, value = br.get(32);
    for (int64_t i = 0; i < n; ++i) {
        const double rng = (double)(high - low) + 1.0, tot = (double)m.c[256];
        const uint32_t T = value - low;
        const uint32_t scaled = (uint32_t)floordiv_big(((double)T + 1.0) * tot - 1.0, rng, 1.0 / rng);
        int s = 0;
        while (m.c[s + 1] <= scaled) ++s;
        narrow(low, high, m.c[s], m.c[s + 1], tot, 1.0 / tot);
        decode_renorm(low, high, value, br);
        m.update(s);
        sym[i] = (uint8_t)s;
    }
}

void cc_floordiv(const double *a, const double *t, double *q, int64_t n)
{
    for (int64_t i = 0; i < n; ++i) q[i] = floordiv(a[i], t[i], 1.0 / t[i]);
}

void cc_floordiv_big(const double *a, const double *t, double *q, int64_t n)
{
    for (int64_t i = 0; i < n; ++i) q[i] = floordiv_big(a[i], t[i], 1.0 / t[i]);
}

}  // extern "C"
