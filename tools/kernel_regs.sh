#!/bin/bash
# Register / spill / kernarg / LDS figures of every kernel in the built libcrt_hip.so: llvm-readelf --notes of EVERY gfx950 code object of
# its fat binary (one per translation unit with kernels; the first is crt_launch.hip's).
set -e
LIB=$(realpath "${1:-$(dirname "$0")/../course-assignment-danielhalachev_amd/libcrt_hip.so}")
LLVM=/opt/rocm/lib/llvm/bin
T=$(mktemp -d)
cp "$LIB" "$T/lib.so"
# llvm-objdump --offloading writes each bundle entry beside its input: lib.so.<n>.<target>
(cd "$T" && $LLVM/llvm-objdump --offloading lib.so > /dev/null)
cd "$T"
for CO in $(ls lib.so.*gfx950* | sort -t. -k3,3n); do
echo "# code object $(echo "$CO" | cut -d. -f3)"
$LLVM/llvm-readelf --notes "$CO" | python3 -c '
import re, sys
txt = sys.stdin.read()
for blk in txt.split("- .agpr_count")[1:]:
    g = lambda k: (re.search(r"\.%s:\s+(\S+)" % k, blk) or [None, "?"])[1]
    name = g("name")
    print("%-70s vgpr %4s sgpr %4s vspill %3s sspill %3s kernarg %5s lds %6s" % (name[:70], g("vgpr_count"), g("sgpr_count"), g("vgpr_spill_count"), g("sgpr_spill_count"), g("kernarg_segment_size"), g("group_segment_fixed_size")))
' | while read -r line; do n=$(echo "$line" | awk '{print $1}'); d=$(c++filt "$n" | sed 's/(anonymous namespace):://; s/((anonymous namespace)::KernelArgs.*//' | cut -c1-60); echo "$d ${line#* }"; done
done
cd /
rm -rf "$T"
