"""Developer utility (CPU): instructions, VGPRs, scratch, LDS and occupancy per kernel of a `hipcc -S --cuda-device-only` listing, demangled.
usage: python tools/isa_table.py FILE.s [--mix] [substring ...]     (--mix: the instruction mix per kernel as well)
A symbol the listing gives no register line for (a device function, not a kernel) prints `-` there."""
import re, subprocess, sys
args = [a for a in sys.argv[1:] if a != "--mix"]
mix = "--mix" in sys.argv[1:]
if not args:
    sys.exit(__doc__)
path, flt = args[0], args[1:]
KINDS = (("valu", ("v_",)), ("pk", ("v_pk_",)), ("ds", ("ds_",)), ("mem", ("global_", "buffer_", "flat_")), ("scratch_ops", ("scratch_",)),
         ("salu", ("s_",)), ("wait", ("s_waitcnt",)))
COUNTED = ("v_", "s_", "ds_", "global_", "buffer_", "flat_", "scratch_")     # n: every instruction once
cur, st = None, {}
for ln in open(path):
    m = re.match(r"^(_ZN3wgs\S+):", ln)
    if m:
        cur = m.group(1); st[cur] = dict(n=0, vgpr="-", scratch="-", lds="-", occ="-", **{k: 0 for k, _ in KINDS}); continue
    if cur is None: continue
    t = ln.strip()
    if t.startswith("; NumVgprs:"): st[cur]["vgpr"] = t.split()[-1]
    elif t.startswith("; ScratchSize:"): st[cur]["scratch"] = t.split()[-1]
    elif t.startswith("; LDSByteSize:"): st[cur]["lds"] = t.split()[2]
    elif t.startswith("; Occupancy:"): st[cur]["occ"] = t.split()[-1]
    elif t.startswith(COUNTED):
        st[cur]["n"] += 1
        for k, prefixes in KINDS:
            if t.startswith(prefixes): st[cur][k] += 1
names = list(st)
dem = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")
for k, dn in zip(names, dem):
    dn = dn.replace("wgs::", "").split("(")[0]
    if not flt or any(f in dn for f in flt):
        v = st[k]
        line = f"{dn[:64]:64s} n={v['n']:5d} vgpr={v['vgpr']:>3s} scratch={v['scratch']:>4s} lds={v['lds']:>6s} occ={v['occ']}"
        if mix:
            line += f" valu={v['valu']:5d} pk={v['pk']:4d} ds={v['ds']:4d} mem={v['mem']:4d} scratch_ops={v['scratch_ops']:4d} salu={v['salu']:5d} wait={v['wait']:4d}"
        print(line)
