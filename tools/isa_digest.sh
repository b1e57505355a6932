#!/bin/bash
# Digest of what the compiler emits for a source tree: the device-only assembly of
# gf_kernels.hip and the host-only assembly of gf_kernels.hip and gf_maps.cpp, built
# with the product flags and a fixed GF_SRC_SHA.  Two trees with equal digests compile
# to the same code (a pure move of text between files leaves them unchanged: no -g, and
# the sources use no __LINE__, __FILE__ or assert).  Compiles only: nothing runs.
#   tools/isa_digest.sh [TREE [EXTRA_FLAGS]]     (TREE defaults to this checkout)
# Keeps the .s files in $ISA_OUT when that is set.
set -e -o pipefail
R=$(cd "${1:-$(dirname "$0")/..}" && pwd)
O=${ISA_OUT:-$(mktemp -d)}
mkdir -p "$O" && O=$(cd "$O" && pwd)
cd "$R/cilium_amd/csrc"      # sources by relative name: the .file line carries no tree path
# -cuid: the compilation-unit id (the name of one marker symbol) is otherwise a hash of the
# source's path and the command line, the output directory included
cc() { hipcc -O3 -std=c++17 --offload-arch=gfx950 -fPIC -Wall -Wno-unused-function -DGF_SRC_SHA='"x"' -cuid=x \
         -Wno-unused-command-line-argument $2 \
         -I "$R/include" -S "$3" -o "$O/$4" "$1"; }
cc --cuda-device-only "$2" gf_kernels.hip device.s &
cc --cuda-host-only "$2" gf_kernels.hip host_kernels.s &
cc --cuda-host-only "$2" gf_maps.cpp host_maps.s &
wait -n; wait -n; wait -n
for f in device.s host_kernels.s host_maps.s; do echo "$f $(sha256sum < "$O/$f" | cut -d' ' -f1)"; done
echo "kernels $(grep -c '^[[:space:]]*\.amdhsa_kernel ' "$O/device.s")"
[ -n "$ISA_OUT" ] || rm -r "$O"
