// vcf_cbaac_coder.h -- one step of the A8 arithmetic coder (the coder behind src/CBAAC.py), written once for
// every tiled CBAAC kernel of vcf_cbaac_gpu.hip and for the host (tests/cpu/cbaac_coder_harness.cpp pins it to
// the serial coder of vcf_cbaac.cpp on the CPU).  The state is the interval [low, high] of 32-bit integers, the
// encoder's count of pending (underflow) bits and the decoder's 32-bit window `value`.  One symbol with
// cumulative counts [lo, hi) of `total` is
//   encoder: narrow, encode_renorm            (encode_flush at the segment's end)
//   decoder: find the symbol, narrow or narrow_floored, decode_renorm
// The model, the decoder's search and the bit I/O are the caller's: a writer offers bits(v, k) and
// run(bit, count), a reader get(k).  Everything compiles for the host and the device and is inlined.
#pragma once

#include <stdint.h>

#include "vcf_dct8.h"   // VCF_HD

#if defined(__HIPCC__)   // VCF_HD for a member function (the host's `static` would make it a static member)
#define VCF_HD_MEMBER __host__ __device__ __forceinline__
#else
#define VCF_HD_MEMBER inline
#endif

namespace vcf {
namespace a8 {

// floor(a / t) for integers a < 2^47, 0 < t <= 2^19 held exactly in doubles,
// given inv ~= 1/t (relative error < 2^-50): q = trunc(a * inv) is within 1
// of the floor, r = a - q t is exact (an fma of integers < 2^47) and lies in
// (-t, 2t), and floor(r * inv + 2^-20) is the step (-1, 0 or +1) that fixes
// q: r / t = m + j/t with j in 0..t-1, and 2^-20 is below 1/t
// (t <= 2^19) and above the error of r * inv.
VCF_HD double floordiv(double a, double t, double inv)
{
    const double q = __builtin_trunc(a * inv);
    const double r = __builtin_fma(-q, t, a);
    return q + __builtin_floor(__builtin_fma(r, inv, 0x1p-20));
}

// floor(a / t) for integers a < 2^47, 1 <= t <= 2^32 held exactly in doubles,
// inv ~= 1/t: the quotient estimate is within one of the floor, the remainder
// (an exact fma) says which way
VCF_HD double floordiv_big(double a, double t, double inv)
{
    const double q = __builtin_trunc(a * inv);
    const double r = __builtin_fma(-q, t, a);
    return r < 0.0 ? q - 1.0 : (r >= t ? q + 1.0 : q);
}

// Interval narrowing from the floored ends ql = floor(range lo / total) and qhm1 = floor(range hi / total) - 1,
// range = high - low + 1: the form of a decoder whose search for the symbol has produced those floors.
VCF_HD void narrow_floored(uint32_t &low, uint32_t &high, uint32_t ql, uint32_t qhm1)
{
    high = low + qhm1;
    low = low + ql;
}

// Interval narrowing to the symbol with cumulative counts [lo, hi) of tot; tot and inv as floordiv takes them.
VCF_HD void narrow(uint32_t &low, uint32_t &high, uint32_t lo, uint32_t hi, double tot, double inv)
{
    const double rng = (double)(high - low) + 1.0;
    const double qh = floordiv(rng * (double)hi, tot, inv);
    const double ql = floordiv(rng * (double)lo, tot, inv);
    const uint32_t qhm1 = (uint32_t)(qh - 1.0);   // before ql's conversion: the order the compiler keeps
    narrow_floored(low, high, (uint32_t)ql, qhm1);
}

// The A8 renormalisation loop in one step.  The loop first shifts out the leading bits that low and high share
// -- d of them (high > low, so d <= 31), the top d bits of low -- and then counts the underflow steps while
// low = 01.. and high = 10..: p of them, each dropping the second bits while the top bits stay 0 and 1.  What
// was shifted out goes to the sink inside the branch that shifts: sink.common(low before the shift, d) if
// d > 0, then sink.underflow(p) if p > 0.  (Handing d, p and the old low back to the caller instead keeps them
// alive across the encoder's stores and turns the shifts into selects: two more VGPRs in the lane encoder.)
template <class Sink>
VCF_HD void renorm(uint32_t &low, uint32_t &high, Sink &&sink)
{
    const uint32_t d = (uint32_t)__builtin_clz(low ^ high);
    if (d) {
        const uint32_t top = low;
        low <<= d;
        high = (high << d) | ((1u << d) - 1u);
        sink.common(top, d);
    }
    const uint32_t x = (low << 1) & ~(high << 1);   // bit 0 is clear: ~x != 0
    const uint32_t p = (uint32_t)__builtin_clz(~x);
    if (p) {
        low = (low << p) & 0x7FFFFFFFu;
        high = (high << p) | ((1u << p) - 1u) | 0x80000000u;
        sink.underflow(p);
    }
}

// The encoder's sink: the first common bit, the pending bits (its opposite), the other d - 1 common bits; the
// underflow steps become pending.
template <class Writer, class Count>
struct Emit {
    Writer &w;
    Count &pending;
    VCF_HD_MEMBER void common(uint32_t top, uint32_t d)
    {
        const uint32_t b = top >> 31;
        w.bits(top, 1);
        w.run(b ^ 1u, pending);
        pending = 0;
        if (d > 1) w.bits(top << 1, d - 1);
    }
    VCF_HD_MEMBER void underflow(uint32_t p) { pending += p; }
};

template <class Writer, class Count>
VCF_HD void encode_renorm(uint32_t &low, uint32_t &high, Count &pending, Writer &w)
{
    renorm(low, high, Emit<Writer, Count>{w, pending});
}

// flush (CBAAC.py:130 -> A8): the bit of low's quarter, then one more pending bit than there are
template <class Writer, class Count>
VCF_HD void encode_flush(Writer &w, uint32_t low, Count pending)
{
    const uint32_t b = low < 0x40000000u ? 0u : 1u;
    w.bits(b << 31, 1);
    w.run(b ^ 1u, pending + 1);
}

// The decoder's sink, its window: d bits shifted in; p more below the top bit, which an underflow step flips.
template <class Reader>
struct Refill {
    uint32_t &value;
    Reader &br;
    VCF_HD_MEMBER void common(uint32_t, uint32_t d) { value = (value << d) | br.get(d); }
    VCF_HD_MEMBER void underflow(uint32_t p) { value = ((value << p) ^ 0x80000000u) | br.get(p); }
};

template <class Reader>
VCF_HD void decode_renorm(uint32_t &low, uint32_t &high, uint32_t &value, Reader &br)
{
    renorm(low, high, Refill<Reader>{value, br});
}

// MSB-first bit writer (bitarray endian='big').  acc holds nb < 32 pending bits at its top; a whole word goes
// to store(index, word) with its bytes swapped, so that a little-endian 32-bit store puts the first bit written
// into the top bit of the first byte.  Store decides who writes it where: one lane of a wave, every lane into
// its own slot, a byte vector on the host.  Count is the type of the word index and of run()'s count: 64 bits
// where the state is wave-uniform (scalar registers), 32 bits in the lane-per-segment encoder, where 64 would
// cost every lane two VGPRs each -- a segment's slot and its pending count stay far below 2^32 bits.
template <class Count, class Store>
struct BitWriter {
    Store store;
    uint64_t acc = 0;
    uint32_t nb = 0;
    Count words = 0;

    VCF_HD_MEMBER void bits(uint32_t v, uint32_t k)   // append the top k bits of v (1 <= k <= 32)
    {
        if (k < 32) v &= ~(0xFFFFFFFFu >> k);
        acc |= (uint64_t)v << (32 - nb);
        nb += k;
        if (nb >= 32) {
            store(words, __builtin_bswap32((uint32_t)(acc >> 32)));
            ++words;
            acc <<= 32;
            nb -= 32;
        }
    }
    VCF_HD_MEMBER void run(uint32_t bit, Count count)
    {
        const uint32_t v = bit ? 0xFFFFFFFFu : 0u;
        for (; count >= 32; count -= 32) bits(v, 32);
        if (count) bits(v, (uint32_t)count);
    }
    VCF_HD_MEMBER uint64_t finish()   // the partial last word, zero padded; returns the bits written in all
    {
        if (nb) store(words, __builtin_bswap32((uint32_t)(acc >> 32)));
        return (uint64_t)words * 32 + nb;
    }
};

}  // namespace a8
}  // namespace vcf
