# developer utility: event-timed passes of several bench configurations (CFGS) for every library variant under tools/tmp_libs/
cp wgsparkl_amd/csrc/libwgsparkl3d_hip.so /tmp/keep.so
for f in tools/tmp_libs/*.so /tmp/keep.so; do
  cp $f wgsparkl_amd/csrc/libwgsparkl3d_hip.so
  for cfg in ${CFGS:-c2 c3 c5}; do
  timeout 120 python bench.py --full --steps 40 --warmup 10 --no-cpu-baseline --no-extra --config $cfg 2>/dev/null | python3 -c "
import sys,json; d=json.loads(sys.stdin.read()); print('$f $cfg', round(d['ms_per_step']*1e3,1), {a:round(b*1e3,1) for a,b in d['pass_ms_per_step'].items() if b>0.0045})"
  done
done
cp /tmp/keep.so wgsparkl_amd/csrc/libwgsparkl3d_hip.so
