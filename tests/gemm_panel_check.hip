// gemm_panel_check.hip — the fp16 similarity panel of k_gemm_nt_ov against the fp32 panel of k_gemm_nt_bf16, through the
// library's own launchers (tests/test_gpu_gemm_panel.py builds and runs it).
//
//   gemm_panel_check <sym|rows> <N> <M> <K> <fp16|bf16>
//
// Seeded operands in [-1, 1] (most of them small, every 37th row eight times larger, so that some sums stay inside
// [-1, 1] and some leave it).  Checks, each printed as "name: ok" or "name: FAIL ...":
//   (a) with clamping on and with clamping off, the fp16 panel is bit for bit the fp32 panel clamped and rounded to the
//       nearest even fp16 on the host;
//   (b) symmetric launches: C[i][j] and C[j][i] are bit-equal;
//   (c) N <= 512: every fp32 entry is within K * 2^-24 * sum |a||b| of the fp64 product of the same operands.
// Exit status 0 when every check passed, 1 when one failed, 2 on a usage or runtime error.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "engine.h"

using namespace knncf;

static uint16_t bits_of(_Float16 h) {
    uint16_t u;
    memcpy(&u, &h, 2);
    return u;
}

// float -> bf16, round to nearest even (the values here are finite)
static uint16_t bf16_bits(float x) {
    uint32_t u;
    memcpy(&u, &x, 4);
    u += 0x7fffu + ((u >> 16) & 1u);
    return (uint16_t)(u >> 16);
}

static float bf16_value(uint16_t b) {
    const uint32_t u = (uint32_t)b << 16;
    float x;
    memcpy(&x, &u, 4);
    return x;
}

int main(int argc, char** argv) {
    if (argc != 6) {
        fprintf(stderr, "usage: gemm_panel_check <sym|rows> <N> <M> <K> <fp16|bf16>\n");
        return 2;
    }
    const bool sym = !strcmp(argv[1], "sym");
    const int64_t N = atoll(argv[2]), M = sym ? N : atoll(argv[3]), K = atoll(argv[4]);
    const bool fp16 = !strcmp(argv[5], "fp16");
    if (N <= 0 || N % 256 || M <= 0 || M % 256 || K <= 0 || K % 64) {
        fprintf(stderr, "gemm_panel_check: N and M must be multiples of 256, K of 64\n");
        return 2;
    }
    int failed = 0;
    try {
        KN_HIP(hipSetDevice(0));
        // operands: B is N x K; the row-block form multiplies its first M rows (A) by all of them
        std::vector<uint16_t> hb((size_t)(N * K));
        std::vector<float> vb((size_t)(N * K));  // the values the device sees
        uint64_t s = 0x9e3779b97f4a7c15ull ^ (uint64_t)(N * 1315423911ll + K * 2654435761ll + (fp16 ? 1 : 2));
        for (int64_t r = 0; r < N; ++r) {
            const float scale = (r % 37 == 5) ? 1.0f : 0.125f;
            for (int64_t c = 0; c < K; ++c) {
                s = s * 6364136223846793005ull + 1442695040888963407ull;
                const float x = ((float)(int32_t)(uint32_t)(s >> 40) * (1.0f / 8388608.0f) - 1.0f) * scale;  // [-1, 1) * scale
                const size_t i = (size_t)(r * K + c);
                if (fp16) {
                    const _Float16 h = (_Float16)x;
                    hb[i] = bits_of(h);
                    vb[i] = (float)h;
                } else {
                    hb[i] = bf16_bits(x);
                    vb[i] = bf16_value(hb[i]);
                }
            }
        }
        DArr<bf16_t> B;
        DArr<_Float16> C16;
        DArr<float> C32;
        DArr<uint32_t> tiles;
        B.alloc(hb.size());
        C16.alloc((size_t)(M * N));
        C32.alloc((size_t)(M * N));
        KN_HIP(hipMemcpy(B.p, hb.data(), hb.size() * 2, hipMemcpyHostToDevice));
        int64_t n_listed = 0;
        if (sym) {
            std::vector<uint32_t> list;
            gemm_sym_tile_list((int32_t)(N / 256), list);
            n_listed = (int64_t)list.size();
            tiles.alloc(list.size());
            KN_HIP(hipMemcpy(tiles.p, list.data(), list.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
        }
        auto launch = [&](void* C, bool c_fp16, bool clamp) {
            if (sym) launch_gemm_sym(B.p, C, c_fp16, N, K, K, N, fp16, clamp, tiles.p, n_listed, nullptr);
            else launch_gemm_nt(B.p, B.p, C, c_fp16, M, N, K, K, K, N, fp16, clamp, nullptr);
            KN_HIP(hipDeviceSynchronize());
        };
        const size_t cells = (size_t)(M * N);
        std::vector<float> h32(cells);
        std::vector<uint16_t> h16(cells);
        KN_HIP(hipMemset(C32.p, 0xff, cells * 4));  // (a NaN: a cell the reference kernel did not write is rejected below)
        launch(C32.p, false, false);
        KN_HIP(hipMemcpy(h32.data(), C32.p, cells * 4, hipMemcpyDeviceToHost));
        {
            size_t nans = 0;
            for (size_t i = 0; i < cells; ++i) nans += h32[i] != h32[i];
            if (nans) {
                ++failed;
                printf("reference: FAIL %zu fp32 cells are NaN (not written)\n", nans);
            } else {
                printf("reference: ok (every fp32 cell written)\n");
            }
        }

        for (int clamp = 1; clamp >= 0; --clamp) {
            KN_HIP(hipMemset(C16.p, 0xff, cells * 2));  // (0xffff is a NaN and the reference holds none: a cell the kernel did not write cannot pass)
            launch(C16.p, true, clamp != 0);
            KN_HIP(hipMemcpy(h16.data(), C16.p, cells * 2, hipMemcpyDeviceToHost));
            const float hi = clamp ? 1.0f : 65504.0f;
            size_t bad = 0, first = 0, clamped = 0, inside = 0;
            for (size_t i = 0; i < cells; ++i) {
                const float x = h32[i];
                const float c = x < -hi ? -hi : (x > hi ? hi : x);
                clamped += c != x;
                inside += std::fabs(x) < 1.0f && x != 0.0f;
                const uint16_t want = bits_of((_Float16)c);
                if (want != h16[i] && !bad++) first = i;
            }
            if (bad) {
                ++failed;
                printf("panel clamp=%d: FAIL %zu of %zu cells differ, first at (%zu, %zu): fp32 %.9g -> %04x, panel %04x\n", clamp, bad,
                       cells, first / (size_t)N, first % (size_t)N, (double)h32[first],
                       bits_of((_Float16)(h32[first] < -hi ? -hi : (h32[first] > hi ? hi : h32[first]))), h16[first]);
            } else {
                printf("panel clamp=%d: ok (%zu cells, %zu beyond the clamp, %zu inside (-1, 1))\n", clamp, cells, clamped, inside);
            }
            if (clamp && (clamped == 0 || inside == 0)) {
                ++failed;
                printf("operands: FAIL the case does not exercise both sides of the clamp\n");
            }
            if (sym) {
                size_t asym = 0, fi = 0, fj = 0;
                constexpr int64_t BL = 64;
                for (int64_t i0 = 0; i0 < N; i0 += BL)
                    for (int64_t j0 = i0; j0 < N; j0 += BL)
                        for (int64_t i = i0; i < i0 + BL; ++i)
                            for (int64_t j = j0; j < j0 + BL; ++j)
                                if (h16[(size_t)(i * N + j)] != h16[(size_t)(j * N + i)] && !asym++) {
                                    fi = (size_t)i;
                                    fj = (size_t)j;
                                }
                if (asym) {
                    ++failed;
                    printf("mirror clamp=%d: FAIL %zu pairs differ, first (%zu, %zu)\n", clamp, asym, fi, fj);
                } else {
                    printf("mirror clamp=%d: ok\n", clamp);
                }
            }
        }
        if (N <= 512) {
            size_t bad = 0;
            double worst = 0.0;
            for (int64_t i = 0; i < M; ++i)
                for (int64_t j = 0; j < N; ++j) {
                    double dot = 0.0, mag = 0.0;
                    for (int64_t c = 0; c < K; ++c) {
                        const double p = (double)vb[(size_t)(i * K + c)] * (double)vb[(size_t)(j * K + c)];
                        dot += p;
                        mag += std::fabs(p);
                    }
                    const double err = std::fabs((double)h32[(size_t)(i * N + j)] - dot), bound = (double)K * 0x1p-24 * mag;
                    if (!(err <= bound)) ++bad;
                    if (mag > 0.0 && err / mag > worst) worst = err / mag;
                }
            if (bad) {
                ++failed;
                printf("fp64: FAIL %zu fp32 entries beyond K * 2^-24 * sum|a||b|\n", bad);
            } else {
                printf("fp64: ok (worst error %.3g of sum|a||b|, bound %.3g)\n", worst, (double)K * 0x1p-24);
            }
        }
    } catch (const Error& e) {
        fprintf(stderr, "gemm_panel_check: %s\n", e.what());
        return 2;
    }
    return failed ? 1 : 0;
}
