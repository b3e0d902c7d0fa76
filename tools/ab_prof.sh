#!/bin/bash
# build with the split-kernel cycle stamps, run tools/split_prof.py on the given shapes, rebuild the default library
ROOT=${GRAFT_REPO_ROOT:-$(pwd)}
cd $ROOT
MEL_HIPCC_FLAGS="-DMEL_GEMM_PROF=99 -DMEL_SPLIT_PROF $EXTRA" python -m melissa_amd.build --force > gpurun_out/prof_build.log 2>&1 || { tail -5 gpurun_out/prof_build.log; exit 1; }
export MEL_HIPCC_FLAGS="-DMEL_GEMM_PROF=99 -DMEL_SPLIT_PROF $EXTRA"
# stop at the first shape that fails or times out (nothing more is started on the GPU after it); the default library comes back either way
status=0
for shape in "$@"; do
    timeout -k 10 120 python tools/split_prof.py $shape 2>&1 | grep -v amdgpu.ids
    status=${PIPESTATUS[0]}
    [ $status -eq 0 ] || { echo "split_prof.py $shape: exit status $status, stopping" >&2; break; }
done
MEL_HIPCC_FLAGS="" python -m melissa_amd.build --force > /dev/null 2>&1
exit $status
