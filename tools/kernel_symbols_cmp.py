#!/usr/bin/env python3
"""Are the kernels of library A still in library B, byte for byte and in the same order?

    tools/kernel_symbols_cmp.py OLD/libwgsparkl3d_hip.so wgsparkl_amd/csrc/libwgsparkl3d_hip.so

Placement alone moves a kernel by a few percent, so a change that only ADDS kernels shows that it left the
measured ones alone: every function symbol of the gfx950 code object of A must exist in B with the same size and the same
bytes, and the symbols of A must come in the same address order in B (new ones may only follow them). Exit status 0 = so.
Needs clang-offload-bundler and llvm-readelf of the ROCm LLVM ($ROCM_PATH/llvm/bin, default /opt/rocm)."""
import os
import subprocess
import sys
import tempfile

LLVM = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin")
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"


def code_object(lib, tmp):
    fatbin, co = os.path.join(tmp, "fat.bin"), os.path.join(tmp, os.path.basename(lib) + ".co")
    subprocess.run([os.path.join(LLVM, "llvm-objcopy"), "-O", "binary", "--only-section=.hip_fatbin", lib, fatbin], check=True)
    subprocess.run([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", f"--targets={TARGET}",
                    f"--input={fatbin}", f"--output={co}"], check=True)
    return co


def functions(co):
    """name -> (address, size, bytes) of the FUNC symbols of .text, and the list of names by address"""
    out = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "-W", "-S", "-s", co], check=True, capture_output=True, text=True).stdout
    text_addr = text_off = None
    for ln in out.splitlines():
        f = ln.replace("[", " ").replace("]", " ").split()
        if len(f) > 5 and f[1] == ".text":
            text_addr, text_off = int(f[3], 16), int(f[4], 16)
    blob = open(co, "rb").read()
    syms = {}
    for ln in out.splitlines():
        f = ln.split()
        if len(f) == 8 and f[3] == "FUNC" and f[6] != "UND":
            addr, size = int(f[1], 16), int(f[2])
            off = addr - text_addr + text_off
            syms[f[7]] = (addr, size, blob[off:off + size])
    return syms, sorted(syms, key=lambda k: syms[k][0])


def main(a, b):
    with tempfile.TemporaryDirectory() as ta, tempfile.TemporaryDirectory() as tb:
        sa, oa = functions(code_object(a, ta))
        sb, ob = functions(code_object(b, tb))
    missing = [k for k in oa if k not in sb]
    resized = [k for k in oa if k in sb and sa[k][1] != sb[k][1]]
    changed = [k for k in oa if k in sb and sa[k][1] == sb[k][1] and sa[k][2] != sb[k][2]]
    # (offsets from the first common symbol: the start of .text itself follows the symbol tables, which grow with every new symbol)
    base_a, base_b = sa[oa[0]][0], sb[oa[0]][0] if oa[0] in sb else 0
    moved = [k for k in oa if k in sb and sa[k][0] - base_a != sb[k][0] - base_b]
    order_ok = [k for k in ob if k in sa] == [k for k in oa if k in sb]
    new = [k for k in ob if k not in sa]
    new_after = not new or not oa or min(sb[k][0] for k in new) > max(sb[k][0] for k in oa if k in sb)
    print(f"{os.path.basename(a)}: {len(oa)} function symbols in A, {len(ob)} in B; missing {len(missing)}, size changed {len(resized)}, "
          f"bytes changed {len(changed)}, address changed {len(moved)}, order kept {order_ok}, {len(new)} new symbols"
          f"{' all behind the old ones' if new_after else ' NOT all behind the old ones'}")
    if changed:   # how much: instruction words that differ (a pc-relative literal that reaches a section behind .text moves with its size)
        words = sum(sum(1 for i in range(0, sa[k][1], 4) if sa[k][2][i:i + 4] != sb[k][2][i:i + 4]) for k in changed)
        print(f"  bytes changed: {words} dwords in {len(changed)} symbols, of {sum(sa[k][1] for k in oa) // 4} dwords")
    for tag, lst in (("missing", missing), ("size", resized), ("bytes", changed), ("address", moved)):
        for k in lst[:8]:
            print(f"  {tag}: {k}")
    return 0 if not (missing or resized or changed or moved) and order_ok and new_after else 1


if __name__ == "__main__":
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    sys.exit(main(sys.argv[1], sys.argv[2]))
