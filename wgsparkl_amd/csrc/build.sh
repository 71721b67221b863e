#!/bin/bash
# Builds the two C-ABI libraries (one per dimension, like the reference's two crates)
# for gfx950 with hipcc. Outputs land next to the sources, libwgsparkl{2,3}d_hip.so, or in $WGS_OUT_DIR (a library variant:
# tools/build_variant.sh; chosen at run time by WGS_LIB_DIR, never copied over the libraries here).
# -ffp-contract=on: multiply-adds are fused where the SOURCE writes them in one expression (a front-end decision),
# never by the back end across statements: the rounding of a kernel body then does not depend on which kernel it is
# compiled into (the paired and the separate launches of a body are bit-identical by construction), and it is
# measurably faster than the default "fast" here (P2G 37 -> 35 us, G2P 43 -> 41 us at C2).
# "Up to date" is decided by content: <lib>.stamp holds a sha256 over the sources, the dimension and the flag line, and a
# library without a matching stamp is rebuilt (a library put there by hand, or built with other WGS_EXTRA_FLAGS, is never
# taken for current). The compiler's version is deliberately left out: a tree carried to another machine with its
# libraries and stamps does not rebuild there. `build.sh force` rebuilds always.
set -euo pipefail
cd "$(dirname "$0")"
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
ARCH=${WGS_ARCH:-gfx950}
FLAGS="-O3 -std=c++17 -fPIC -shared --offload-arch=${ARCH} -fno-fast-math -ffp-contract=on -Wall -Wno-unused-variable -Wno-unused-but-set-variable -Wno-unused-value -Wno-unused-result ${WGS_EXTRA_FLAGS:-}"
# (the in-tree compile line stays exactly `-o libwgsparkl<dim>d_hip.so.tmp`: hipcc hashes its command line into the
# library's __hip_cuid_* symbol, so another spelling of the same path gives other bytes around the same code object)
OUT=${WGS_OUT_DIR:+$WGS_OUT_DIR/}
[[ -n "$OUT" ]] && mkdir -p "$OUT"
sources=$(sha256sum capi.hip *.h *.inc ../../include/wgsparkl_hip.h ../../include/wgsparkl_hip_forces.h ../../include/wgsparkl_hip_emit.h ../../include/wgsparkl_hip_remove.h)
pids=()
for dim in 3 2; do
  out="${OUT}libwgsparkl${dim}d_hip.so"
  stamp=$(printf '%s\ndim=%s\nflags=%s\n' "$sources" "$dim" "$FLAGS" | sha256sum | cut -d' ' -f1)
  if [[ "${1:-}" != "force" && -f "$out" && -f "$out.stamp" && "$(cat "$out.stamp")" == "$stamp $(sha256sum < "$out" | cut -d' ' -f1)" ]]; then
    continue
  fi
  rm -f "$out.stamp"
  { $HIPCC $FLAGS -DWGS_DIM=$dim capi.hip -o "$out.tmp" && mv "$out.tmp" "$out" && echo "$stamp $(sha256sum < "$out" | cut -d' ' -f1)" > "$out.stamp"; } &
  pids+=($!)
done
rc=0
for p in "${pids[@]:-}"; do [[ -n "$p" ]] && { wait "$p" || rc=1; }; done
exit $rc
