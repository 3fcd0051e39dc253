# usage (GPU box, repo root): bash scripts/gemm_variants.sh "<k list>" "<flags of variant 1>" "<flags of variant 2>" ...
# A/B of compile-time variants of the similarity GEMM alone (scripts/microbench/gemm_bench.hip): rebuilds the library per
# flag set and the benchmark against it.
KS=$1; shift
LIB=$PWD/movie-recommender-system_amd
for FLAGS in "$@"; do
  KNNCF_EXTRA_HIPCC_FLAGS="$FLAGS" python -c "
import importlib
importlib.import_module('movie-recommender-system_amd.build').build(force=True)" || exit 1
  hipcc --offload-arch=gfx950 -O2 -std=c++17 -I $LIB/csrc scripts/microbench/gemm_bench.hip -L $LIB -lknncf -Wl,-rpath,$LIB \
        -o /tmp/gemm_bench || exit 1
  echo "== [$FLAGS]"
  /tmp/gemm_bench --k $KS 2>&1 | grep -v amdgpu.ids
done
