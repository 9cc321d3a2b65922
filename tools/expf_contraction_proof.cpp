// expf_contraction_proof.cpp -- host proof behind the Horner form of exact_expf / exact_expf_select (csrc/mnv_device.h).
//
// glibc 2.35's expf evaluates its degree-3 polynomial without fused operations:
//     z = C0*r + C1;  r2 = r*r;  y = C2*r + 1;  y = z*r2 + y;  y = y*s;  return (float)y
// in binary64.  This program runs every binary32 input that reaches that polynomial (all 2^32 bit patterns are visited; the ones that
// leave through a special case before it are counted and skipped, they never see the polynomial) and compares the result bits of that
// evaluation with five others:
//     1  z = fma(C0, r, C1)                    2  y = fma(C2, r, 1)                    3  y = fma(z, r2, y)
//     4  all three of them                     5  Horner: fma(fma(fma(C0, r, C1), r, C2), r, 1) * s     (what the kernels run)
// A sixth evaluation is a control that MUST differ (the polynomial on r rounded to binary32): it shows that the comparison is live.
// The C library's own expf is compared as well and only reported (it may be any algorithm).
//
// Prints one line per count; exit status 0 when the five variants have no mismatch and the control has some, 1 otherwise.
// Build: c++ -O2 -std=c++17 -ffp-contract=off -pthread tools/expf_contraction_proof.cpp -o expf_proof   (+ -march=native for a hardware fma)
// Threads: OMP_NUM_THREADS, default 4.
#include <atomic>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <vector>

namespace {

const uint64_t kTab[32] = {
    0x3ff0000000000000ULL, 0x3fefd9b0d3158574ULL, 0x3fefb5586cf9890fULL, 0x3fef9301d0125b51ULL, 0x3fef72b83c7d517bULL, 0x3fef54873168b9aaULL,
    0x3fef387a6e756238ULL, 0x3fef1e9df51fdee1ULL, 0x3fef06fe0a31b715ULL, 0x3feef1a7373aa9cbULL, 0x3feedea64c123422ULL, 0x3feece086061892dULL,
    0x3feebfdad5362a27ULL, 0x3feeb42b569d4f82ULL, 0x3feeab07dd485429ULL, 0x3feea47eb03a5585ULL, 0x3feea09e667f3bcdULL, 0x3fee9f75e8ec5f74ULL,
    0x3feea11473eb0187ULL, 0x3feea589994cce13ULL, 0x3feeace5422aa0dbULL, 0x3feeb737b0cdc5e5ULL, 0x3feec49182a3f090ULL, 0x3feed503b23e255dULL,
    0x3feee89f995ad3adULL, 0x3feeff76f2fb5e47ULL, 0x3fef199bdd85529cULL, 0x3fef3720dcef9069ULL, 0x3fef5818dcfba487ULL, 0x3fef7c97337b9b5fULL,
    0x3fefa4afa2a490daULL, 0x3fefd0765b6e4540ULL,
};

constexpr double N = 32.0;
constexpr double InvLn2N = 0x1.71547652b82fep+0 * N;
constexpr double SHIFT = 0x1.8p+52;
constexpr double C0 = 0x1.c6af84b912394p-5 / N / N / N;
constexpr double C1 = 0x1.ebfce50fac4f3p-3 / N / N;
constexpr double C2 = 0x1.62e42ff0c52d6p-1 / N;

constexpr int kVariants = 6;  // 0-4: the five candidates, 5: the control

uint32_t bits_of(float v) {
    uint32_t u;
    std::memcpy(&u, &v, 4);
    return u;
}

// true when x leaves exact_expf before the polynomial
bool special(uint32_t ix, float x) {
    const uint32_t abstop = (ix >> 20) & 0x7ffu;
    if (abstop >= 0x42bu) {
        if (ix == 0xff800000u) return true;
        if (abstop >= 0x7f8u) return true;
        if (x > 0x1.62e42ep6f) return true;
        if (x < -0x1.9fe368p6f) return true;
    }
    return false;
}

struct Counts {
    uint64_t main_path = 0, mismatch[kVariants] = {}, libm = 0;
};

void run(uint64_t first, uint64_t last, Counts *out) {
    Counts c;
    for (uint64_t p = first; p < last; ++p) {
        const uint32_t ix = (uint32_t)p;
        float x;
        std::memcpy(&x, &ix, 4);
        if (special(ix, x)) continue;
        ++c.main_path;
        const double xd = (double)x;
        double z = InvLn2N * xd;
        double kd = z + SHIFT;
        uint64_t ki;
        std::memcpy(&ki, &kd, 8);
        kd -= SHIFT;
        const double r = z - kd;
        uint64_t t = kTab[ki & 31u];
        t += ki << 47;
        double s;
        std::memcpy(&s, &t, 8);
        const double r2 = r * r;
        // the evaluation of glibc 2.35 (this file is compiled with -ffp-contract=off: nothing fuses by itself)
        const double z0 = C0 * r + C1;
        const double y0 = C2 * r + 1.0;
        const uint32_t want = bits_of((float)((z0 * r2 + y0) * s));
        const double zf = std::fma(C0, r, C1), yf = std::fma(C2, r, 1.0);
        const double rf = (double)(float)r;
        const float got[kVariants] = {
            (float)((zf * r2 + y0) * s),
            (float)((z0 * r2 + yf) * s),
            (float)(std::fma(z0, r2, y0) * s),
            (float)(std::fma(zf, r2, yf) * s),
            (float)(std::fma(std::fma(std::fma(C0, r, C1), r, C2), r, 1.0) * s),
            (float)(((C0 * rf + C1) * (rf * rf) + (C2 * rf + 1.0)) * s),
        };
        for (int v = 0; v < kVariants; ++v) c.mismatch[v] += bits_of(got[v]) != want;
        c.libm += bits_of(expf(x)) != want;
    }
    *out = c;
}

}  // namespace

int main() {
    int threads = 4;
    if (const char *e = getenv("OMP_NUM_THREADS")) threads = atoi(e);
    if (threads < 1) threads = 1;
    if (threads > 256) threads = 256;
    // interleaved 2^20-pattern blocks, so that every thread gets its share of the special ranges
    const uint64_t kBlock = 1ull << 20, kBlocks = 1ull << 12;
    std::vector<Counts> part(threads);
    std::vector<std::thread> pool;
    for (int w = 0; w < threads; ++w) {
        pool.emplace_back([&, w]() {
            Counts sum;
            for (uint64_t b = (uint64_t)w; b < kBlocks; b += (uint64_t)threads) {
                Counts c;
                run(b * kBlock, (b + 1) * kBlock, &c);
                sum.main_path += c.main_path;
                sum.libm += c.libm;
                for (int v = 0; v < kVariants; ++v) sum.mismatch[v] += c.mismatch[v];
            }
            part[w] = sum;
        });
    }
    for (auto &t : pool) t.join();
    Counts all;
    for (const Counts &c : part) {
        all.main_path += c.main_path;
        all.libm += c.libm;
        for (int v = 0; v < kVariants; ++v) all.mismatch[v] += c.mismatch[v];
    }
    static const char *const names[kVariants] = {"fma_z", "fma_y", "fma_last", "fma_all", "horner", "control_r_binary32"};
    printf("patterns %llu\n", 1ull << 32);
    printf("main_path %llu\n", (unsigned long long)all.main_path);
    bool ok = all.main_path > 0;
    for (int v = 0; v < kVariants; ++v) {
        printf("mismatch_%s %llu\n", names[v], (unsigned long long)all.mismatch[v]);
        ok = ok && (v == kVariants - 1 ? all.mismatch[v] != 0 : all.mismatch[v] == 0);
    }
    printf("mismatch_libm_expf %llu\n", (unsigned long long)all.libm);
    printf(ok ? "PROOF HOLDS\n" : "PROOF FAILS\n");
    return ok ? 0 : 1;
}
