// gemm_bench.hip — the similarity GEMM alone: ms per launch of the symmetric form (default) or of the row-block form
// (--rows M) at N users x K head columns, fp16 operands and panel, through the library's own launchers (launch_gemm_sym /
// launch_gemm_nt).  Build + run (GPU box):
//   hipcc --offload-arch=gfx950 -O2 -std=c++17 -I movie-recommender-system_amd/csrc scripts/microbench/gemm_bench.hip \
//         -L movie-recommender-system_amd -lknncf -Wl,-rpath,$PWD/movie-recommender-system_amd -o /tmp/gemm_bench && \
//   /tmp/gemm_bench [--n 162560] [--k 384,512,768] [--rows 0 (symmetric) | M] [--iters 5]
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "engine.h"

using namespace knncf;

// the operand panel: a cheap pattern, values in [-1/16, 1/16] (the MFMA rate does not depend on the data, the chip's clock
// under load does a little)
__global__ void k_fill(bf16_t* p, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) reinterpret_cast<_Float16*>(p)[i] = (_Float16)((float)((int)((i * 2654435761u) >> 20 & 255) - 128) * (1.0f / 2048.0f));
}

// ms per launch: the symmetric form (rows == 0: all N rows) or the row-block form (rows M), after one warm-up launch
static double ms_per_launch(int64_t N, int64_t K, int64_t rows, int iters) {
    const bool sym = rows == 0;
    DArr<bf16_t> B;
    DArr<_Float16> C;
    DArr<uint32_t> tiles;
    B.alloc((size_t)(N * K));
    C.alloc((size_t)((sym ? N : rows) * N));
    k_fill<<<(unsigned)ceil_div(N * K, 256), 256>>>(B.p, N * K);
    KN_HIP(hipGetLastError());
    int64_t n_listed = 0;
    if (sym) {
        std::vector<uint32_t> list;
        gemm_sym_tile_list((int32_t)(N / 256), list);
        n_listed = (int64_t)list.size();
        tiles.alloc(list.size());
        KN_HIP(hipMemcpy(tiles.p, list.data(), list.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    }
    auto once = [&] {
        if (sym) launch_gemm_sym(B.p, C.p, true, N, K, K, N, true, true, tiles.p, n_listed, nullptr);
        else launch_gemm_nt(B.p, B.p, C.p, true, rows, N, K, K, K, N, true, true, nullptr);
    };
    hipEvent_t a, b;
    KN_HIP(hipEventCreate(&a));
    KN_HIP(hipEventCreate(&b));
    once();
    KN_HIP(hipDeviceSynchronize());
    KN_HIP(hipEventRecord(a, nullptr));
    for (int i = 0; i < iters; ++i) once();
    KN_HIP(hipEventRecord(b, nullptr));
    KN_HIP(hipEventSynchronize(b));
    float ms = 0.f;
    KN_HIP(hipEventElapsedTime(&ms, a, b));
    (void)hipEventDestroy(a);
    (void)hipEventDestroy(b);
    return (double)ms / iters;
}

static int usage() {
    fprintf(stderr, "usage: gemm_bench [--n 162560] [--k 384[,512,...]] [--rows 0 (symmetric) | M] [--iters 5]\n"
                    "  N and M multiples of 256, every K a multiple of 64\n");
    return 2;
}

int main(int argc, char** argv) {
    int64_t n = 162560, rows = 0;
    int iters = 5;
    std::string k_list = "384";
    for (int i = 1; i < argc; ++i) {
        if (i + 1 >= argc) return usage();
        const char* v = argv[++i];
        if (!strcmp(argv[i - 1], "--n")) n = atoll(v);
        else if (!strcmp(argv[i - 1], "--k")) k_list = v;
        else if (!strcmp(argv[i - 1], "--rows")) rows = atoll(v);
        else if (!strcmp(argv[i - 1], "--iters")) iters = atoi(v);
        else return usage();
    }
    std::vector<int64_t> ks;
    for (size_t p = 0; p < k_list.size();) {
        const size_t q = std::min(k_list.find(',', p), k_list.size());
        ks.push_back(atoll(k_list.substr(p, q - p).c_str()));
        p = q + 1;
    }
    if (n <= 0 || n % 256 || rows < 0 || rows % 256 || iters <= 0 || ks.empty()) return usage();
    for (int64_t k : ks)
        if (k <= 0 || k % 64) return usage();
    try {
        KN_HIP(hipSetDevice(0));
        for (int64_t k : ks) {
            const double ms = ms_per_launch(n, k, rows, iters);
            const int64_t m = rows ? rows : n;
            // executed flops: the tiles on and above the diagonal (symmetric) or all of them, 2 per multiply-add
            const double flops = (rows ? 2.0 * (double)rows * (double)n : (double)n * (double)(n + 256)) * (double)k;
            const double panel = (double)m * (double)n * 2.0;
            printf("N %lld K %lld rows %lld %s: %8.3f ms/launch  %7.1f TFLOP/s executed  panel %.1f GB -> %.2f TB/s written\n",
                   (long long)n, (long long)k, (long long)m, rows ? "row-block" : "sym", ms, flops / ms / 1e9, panel / 1e9,
                   panel / ms / 1e9);
            fflush(stdout);
        }
    } catch (const Error& e) {
        fprintf(stderr, "gemm_bench: %s\n", e.what());
        return 1;
    }
    return 0;
}
