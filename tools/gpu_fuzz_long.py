"""Developer utility: many more seeds of the fuzz parity tests than the suite runs (bug hunting on an idle GPU)."""
import sys, traceback; sys.path.insert(0, '.'); sys.path.insert(0, 'tests')
import numpy as np
import gpu_common as T
from helpers import run_gpu, run_oracle, rel_rms
lo, hi = int(sys.argv[1]), int(sys.argv[2])
bad = []
for seed in range(lo, hi):
    try:
        sc = T._random_scene(seed)
        k = int(sys.argv[3]) if len(sys.argv) > 3 else 12
        chunk = int(sys.argv[4]) if len(sys.argv) > 4 else 0
        if chunk:      # the same substeps in several calls with a wgs_sync between them: the launch shapes that follow the
            from helpers import pipeline                     # near-collider list the host last saw get exercised
            from wgsparkl_amd import MpmData
            pipe = pipeline(sc["particles"].dim)
            data = MpmData.from_scene(pipe, sc)
            done = 0
            while done < k:
                pipe.step(data, min(chunk, k - done)); data.sync(); done += chunk
        else:
            data = run_gpu(sc, k)
        st, st64 = run_oracle(sc, k, np.float32), run_oracle(sc, k, np.float64)
        cells, vm, dist, aff, closest = data.read_grid()
        oc, omv, odist, oaff, oclosest = st.grid_records()
        assert cells.shape == oc.shape and (np.array_equal(cells, oc) or k > 12), "cells"
        assert (aff != oaff).mean() < 0.005, "aff"
        got = data.read_particles()
        same = got.cdf_affinity == st.arr["cdf_affinity"]
        assert same.mean() > 0.99, "paff"
        for f, tol in (("pos", 2e-5), ("vel", 2e-3)):
            err = rel_rms(getattr(got, f)[same], st64.arr[f][same]); err32 = rel_rms(st.arr[f][same], st64.arr[f][same])
            assert err < max(tol, 10.0 * err32) * (1.0 if k <= 12 else 50.0), (f, err, err32)
        if sc["colliders"]:
            st.update_world_mass_properties()
            for gb, ob in zip(data.read_body_poses(), st.collider_states()):
                for key in ("rotation", "translation", "linvel", "angvel"):
                    assert np.allclose(gb[key], ob[key], rtol=0.0, atol=2e-3 if k <= 12 else 5e-2), (key, gb[key], ob[key])
    except Exception as e:  # noqa: BLE001
        bad.append((seed, repr(e)[:200]))
print("seeds", lo, hi, "failures:", bad)
