#!/bin/bash
# Debug build for tools/gemm_timeline.py: gemm256.hip with -DMHMR_GEMM_STAMPS linked against the product's other objects
# (run `python -c "import __graft_entry__ as g; g.build()"` first).  Output: tools/dbg/libmhmr_gemm_stamps.so (git-ignored).
set -e
R=$(cd "$(dirname "$0")/.." && pwd)
C=$R/multi_hmr_amd/csrc
mkdir -p $R/tools/dbg
# the product's own flags (multi_hmr_amd/_lib.py), so that this object matches the ones it is linked against
FLAGS=$(cd $R && python -c "from multi_hmr_amd import _lib; print(' '.join(_lib.COMMON_FLAGS + _lib.EXTRA_FLAGS.get('gemm256.hip', [])))")
/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC $FLAGS -DMHMR_GEMM_STAMPS -c $C/gemm256.hip -o /tmp/gemm256_stamps.o
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o $R/tools/dbg/libmhmr_gemm_stamps.so /tmp/gemm256_stamps.o $(ls $C/build/*.o | grep -v "/gemm256.o")
echo built $R/tools/dbg/libmhmr_gemm_stamps.so
