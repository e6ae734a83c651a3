// Host-side exercise of csrc/operand_split.h for tests/test_operand_split_host.py: compiled with hipcc --cuda-host-only, run on
// the CPU, prints one "key value" line per finding.  The bounds themselves are asserted by the Python test.
#include "operand_split.h"
#include <math.h>
#include <stdint.h>
#include <stdio.h>

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rng() {                                   // splitmix64
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
// a value with a random sign and significand and an exponent drawn evenly from [elo, ehi]: |v| in [2^elo, 2^(ehi + 1))
static float draw(int elo, int ehi) {
    const uint64_t r = rng();
    const unsigned e = (unsigned)(127 + elo + (int)((r >> 32) % (uint64_t)(ehi - elo + 1)));
    return __builtin_bit_cast(float, (unsigned)((r >> 63) << 31) | (e << 23) | (unsigned)(r & 0x7FFFFFu));
}
static float bf16_value(unsigned half) { return __builtin_bit_cast(float, half << 16); }
static double f16_value(unsigned half) { return (double)__builtin_bit_cast(_Float16, (unsigned short)half); }
static bool same_bits(float a, float b) { return __builtin_bit_cast(unsigned, a) == __builtin_bit_cast(unsigned, b); }

// worst |hi + lo - v| over both halves of n pairs with exponents in [elo, ehi], relative to |v| or absolute
static double np2_worst(int n, int elo, int ehi, bool relative) {
    double worst = 0.0;
    for (int i = 0; i < n; ++i) {
        const float v[2] = {draw(elo, ehi), draw(elo, ehi)};
        unsigned o[2];
        split_pair<2>(v[0], v[1], o);
        for (int half = 0; half < 2; ++half) {
            const unsigned sh = 16 * half;
            const double err = fabs(f16_value((o[0] >> sh) & 0xFFFFu) + f16_value((o[1] >> sh) & 0xFFFFu) - (double)v[half]);
            worst = fmax(worst, relative ? err / fabs((double)v[half]) : err);
        }
    }
    return worst;
}

template <int TOP, class Scale>
static void check_scale(const char* name, Scale scale) {
    int checked = 0, bad = 0;
    for (unsigned eb = 0; eb < 256; ++eb) {
        const unsigned mant[4] = {0u, 1u, 0x7FFFFFu, (unsigned)(rng() & 0x7FFFFFu)};      // (eb 0: zero, denormals; eb 255: inf, NaNs)
        for (int k = 0; k < 4; ++k) {
            const float m = __builtin_bit_cast(float, (eb << 23) | mant[k]);
            float S = 0.f, invS = 0.f;
            scale(m, S, invS);
            bool ok;
            if (eb >= 16u && eb <= 250u) ok = m * S >= ldexpf(1.f, TOP) && m * S < ldexpf(1.f, TOP + 1) && S * invS == 1.f;
            else ok = same_bits(S, 1.f) && same_bits(invS, 1.f);
            ++checked;
            bad += !ok;
        }
    }
    printf("%s_checked %d\n%s_bad %d\n", name, checked, name, bad);
}

template <int NP>
static int quad_mismatches(int n) {
    int bad = 0;
    for (int i = 0; i < n; ++i) {
        const float e[4] = {draw(-27, 14), draw(-27, 14), draw(-27, 14), draw(-27, 14)};
        uint2 o[NP];
        unsigned a[NP], b[NP];
        split_quad<NP>(e, o);
        split_pair<NP>(e[0], e[1], a);
        split_pair<NP>(e[2], e[3], b);
        for (int pp = 0; pp < NP; ++pp) bad += o[pp].x != a[pp] || o[pp].y != b[pp];
    }
    return bad;
}

int main() {
    // NP = 3: the low halves sum to the first argument, the high halves to the second, bit for bit
    {
        const int n = 1000000;
        int bad_lo = 0, bad_hi = 0;
        for (int i = 0; i < n; ++i) {
            const float a = draw(-27, 22), b = draw(-27, 22);
            unsigned o[3], h, m, l;
            split_pair<3>(a, b, o);
            split_pair(a, b, h, m, l);
            const float sa = (bf16_value(o[0] & 0xFFFFu) + bf16_value(o[1] & 0xFFFFu)) + bf16_value(o[2] & 0xFFFFu);
            const float sb = (bf16_value(o[0] >> 16) + bf16_value(o[1] >> 16)) + bf16_value(o[2] >> 16);
            bad_lo += !same_bits(sa, a) || h != o[0];
            bad_hi += !same_bits(sb, b) || m != o[1] || l != o[2];
        }
        printf("np3_values %d\nnp3_bad_lo %d\nnp3_bad_hi %d\n", n, bad_lo, bad_hi);
    }
    // NP = 2 on magnitudes the caller has scaled: 22 bits where |v| is within 2^16 of 2^14, an absolute bound below
    printf("np2_rel_values %d\nnp2_rel_worst_log2 %.6f\n", 4000000, log2(np2_worst(2000000, -2, 14, true)));
    printf("np2_abs_values %d\nnp2_abs_worst_log2 %.6f\n", 1000000, log2(np2_worst(500000, -40, -3, false)));
    check_scale<14>("block_scale", [](float m, float& S, float& invS) { block_scale(m, S, invS); });
    check_scale<12>("weight_scale", [](float m, float& S, float& invS) { weight_scale(m, S, invS); });
    printf("quad3_bad %d\nquad2_bad %d\n", quad_mismatches<3>(100000), quad_mismatches<2>(100000));
    return 0;
}
