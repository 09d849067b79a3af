#!/bin/bash
# usage: tools/mk.sh <output.so> [extra hipcc flags]  -- builds libhssfsst with the release flags of _lib.build() (from anywhere; a relative
# output path is taken from the current directory): the units of _lib.SOURCES, concurrently, each into an object under <output.so>.objs/,
# then the link; prints VGPRs, scratch bytes per lane and SGPR spills of every kernel
set -o pipefail
out=$1; shift
R=$(cd "$(dirname "$0")/.." && pwd)                     # the repository this script lives in
srcs=$(cd "$R" && python3 -c "from heart_sounds_segmentation_amd import _lib; print('\n'.join(_lib.SOURCES))") || exit 1
mkdir -p "$out.objs" || exit 1
objs=()
for src in $srcs; do
    obj="$out.objs/$(basename "${src%.hip}").o"; objs+=("$obj")
    hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC "$@" -c -o "$obj" "$src" -Rpass-analysis=kernel-resource-usage > "$obj.log" 2>&1 &
done
wait
{ cat "${objs[@]/%/.log}"; hipcc --offload-arch=gfx950 -shared -fPIC -o "$out" "${objs[@]}" 2>&1; } |
    grep -E "error|Function Name|VGPRs:|ScratchSize|SGPRs Spill" | grep -v "AGPRs\|VGPRs Spill" | sed 's/.*remark: *//; s/ \[-Rpass.*//' |
    awk '/error/{print} /Function Name/{n=$3} /^ *VGPRs:/{v=$2} /ScratchSize/{sc=$3} /SGPRs Spill/{printf "%-100s vgpr %3s scratch %4s sgpr-spill %s\n", substr(n,1,100), v, sc, $3}' |
    sed 's/_ZN7hssfsst//'
