#!/bin/sh
# VGPRs, scratch bytes and waves per SIMD of every kernel of one translation unit of omni-pq_amd/csrc, as the compiler reports
# them (-Rpass-analysis=kernel-resource-usage), compiled with the flags omni-pq_amd/build.py uses.  Device code only: nothing
# is linked or written.
#     tools/probe/spills.sh optim.hip [pattern of the kernels' mangled names, e.g. adamw_update]
set -e
here=$(cd "$(dirname "$0")/../.." && pwd)
src=${1:?usage: spills.sh FILE.hip [pattern]}
pattern=${2:-.}
flags=$(cd "$here/omni-pq_amd" && python -c "import build, sys; print(' '.join(build.COMMON + build.EXTRA.get(sys.argv[1], [])))" "$src")
hipcc=$(cd "$here/omni-pq_amd" && python -c "import build; print(build.hipcc())")
# shellcheck disable=SC2086
"$hipcc" $flags --cuda-device-only -c -o /dev/null -Rpass-analysis=kernel-resource-usage "$here/omni-pq_amd/csrc/$src" 2>&1 |
    sed -n -e 's/ \[-Rpass-analysis=kernel-resource-usage\]//' -e 's/^.*remark: //p' |
    awk -v pat="$pattern" '/^Function Name:/ { show = ($0 ~ pat) } show && /Function Name:|^ *VGPRs:|ScratchSize|Occupancy/'
