"""-m "not gpu": the multi-GPU substep protocol (wgsparkl_amd/csrc/kernels_shard.h) restated on the CPU oracle
(tests/shard_oracle.py) under torch.distributed with the gloo backend, world_size 2 and 3: the decomposed run must
reproduce the single-domain oracle run (fp64, so only the association of the interface sums differs)."""
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


def test_partition_helpers():
    from wgsparkl_amd.sharded import INT_MAX, INT_MIN, SlabPartition
    p = SlabPartition([0, 4, 9, 12])
    assert p.world == 3
    assert p.block_range(0) == (INT_MIN, 4) and p.block_range(1) == (4, 9) and p.block_range(2) == (9, INT_MAX)
    assert p.owner_of_blocks(np.array([-5, 0, 3, 4, 8, 9, 100])).tolist() == [0, 0, 0, 1, 1, 2, 2]
    bx = np.repeat(np.arange(10), 100)
    q = SlabPartition.balanced(bx, 4)
    counts = np.bincount(q.owner_of_blocks(bx), minlength=4)
    assert counts.min() >= 200 and counts.sum() == 1000


@pytest.mark.parametrize("dim,world,k", [(3, 2, 20), (2, 2, 20), (3, 3, 20)])
def test_gloo_matches_single_domain(oracle_libs, tmp_path, dim, world, k):
    """world_size 2 and 3 (an interior slab with two neighbours) over gloo: the one-exchange protocol — guests transferred
    to the grid by their old owner, advanced by their new owner from the message — reproduces the single-domain run."""
    out = str(tmp_path / "shard")
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(29611 + dim + 10 * world), WORLD_SIZE=str(world), OMP_NUM_THREADS="1")
    procs = [subprocess.Popen([sys.executable, os.path.join(HERE, "shard_gloo_worker.py"), str(dim), str(k), out],
                              env=dict(env, RANK=str(r)), stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
             for r in range(world)]
    logs = [p.communicate(timeout=600)[0].decode() for p in procs]
    assert all(p.returncode == 0 for p in procs), "\n".join(logs)
    res = [np.load(f"{out}.rank{r}.npz") for r in range(world)]

    sys.path.insert(0, HERE)
    from shard_gloo_worker import make_scene
    from wgsparkl_amd.selfcheck import rel_rms
    from wgsparkl_amd.sharded import join_slabs
    sc = make_scene(dim, world)
    ps = sc["particles"]
    st = oracle_libs.Oracle(dim, np.float64).new_state(ps, sc["params"], sc["colliders"], sc["cell_width"],
                                                       sc["grid_capacity"], sc.get("model", 0))
    st.step(k)
    joined = join_slabs(res, np.arange(ps.n), fields=("pos", "vel", "def_grad", "affine"))
    assert joined.exact, joined.problem                                     # nobody lost, nobody duplicated
    assert joined.counts != [int(r["n0"][0]) for r in res]                  # particles did migrate
    for f, got in joined.fields.items():
        err = rel_rms(got, st.arr[f])
        assert err < 1e-9, (f, err)


def test_protocol_lockstep_four_slabs_and_mask_table(oracle_libs):
    """The same restated protocol with all ranks in one process (4 slabs: two interior ones), and the interface masks it
    shares with kernels_shard.h spelt out for one slab."""
    sys.path.insert(0, HERE)
    from shard_gloo_worker import make_scene, partition_of
    from shard_oracle import OracleShard, iface_masks, lockstep
    from wgsparkl_amd.selfcheck import rel_rms
    from wgsparkl_amd.sharded import join_slabs, split_scene
    # rank with core range [8, 12), both neighbours, 3D (2 x-layer pairs per block): what each layer is to it
    m = {bx: iface_masks(bx, 8, 12, True, True, 2) for bx in range(6, 15)}      # (recv, send_lo, send_hi)
    assert m[6] == (0, 0, 0) and m[14] == (0, 0, 0) and m[10] == (0, 0, 0)
    assert m[7] == (0, 3, 0)          # layer lo - 1: only guests write it; everything they wrote goes down
    assert m[8] == (3, 1, 0)          # layer lo: first pair shared with the lower neighbour's core; all pairs may receive
    assert m[9] == (1, 0, 0)          # layer lo + 1: first pair may receive (the lower neighbour's guests)
    assert m[11] == (3, 0, 0)         # layer hi - 1: may receive (the upper neighbour's guests)
    assert m[12] == (1, 0, 3)         # layer hi: own core reaches the first pair, own guests all of it: all pairs go up
    assert m[13] == (0, 0, 1)         # layer hi + 1: own guests reach the first pair
    world, k = 4, 12
    sc = make_scene(3, world)
    part = partition_of(sc, world)
    assert part.min_interior_width() >= 3
    shards = []
    for r, (sub, gids) in enumerate(split_scene(sc["particles"], part, sc["cell_width"])):
        lo, hi = part.block_range(r)
        shards.append(OracleShard(sc, sub, gids, lo, hi, r > 0, r < world - 1))
    n0 = [len(s.gids) for s in shards]
    lockstep(shards, k)
    st = oracle_libs.Oracle(3, np.float64).new_state(sc["particles"], sc["params"], sc["colliders"], sc["cell_width"], sc["grid_capacity"], sc.get("model", 0))
    st.step(k)
    joined = join_slabs([s.export() for s in shards], np.arange(sc["particles"].n), fields=("pos", "vel", "def_grad", "affine"))
    assert joined.exact and joined.counts != n0, joined.problem
    for f, got in joined.fields.items():
        assert rel_rms(got, st.arr[f]) < 1e-9, f


def _hand_made_exports(dim, ids_per_rank):
    """export()-shaped dicts of hand-made "ranks": every value of a particle's fields is a function of its id alone"""
    def one(ids):
        ids = np.asarray(ids, np.uint32)
        base = ids.astype(np.float32)[:, None]
        return dict(ids=ids, pos=base + np.arange(dim, dtype=np.float32) / 8, def_grad=100 * base + np.arange(dim * dim, dtype=np.float32),
                    mass=base[:, 0] + 0.5)
    return [one(ids) for ids in ids_per_rank]


@pytest.mark.parametrize("dim", [2, 3])
def test_join_slabs_orders_by_id_and_names_what_is_wrong(dim):
    """sharded.join_slabs on three hand-made ranks: fields in id order with holder and counts; an empty rank; a missing id and an id
    on two ranks named in `problem`; an expected id set that is not arange; a non-particle entry selected away by `fields`."""
    from wgsparkl_amd.sharded import join_slabs
    per_rank = [[7, 2, 9], [0, 8, 4, 1], [5, 3, 6]]
    j = join_slabs(_hand_made_exports(dim, per_rank))
    assert j.exact and j.counts == [3, 4, 3] and j.ids.tolist() == list(range(10))
    assert j.holder.tolist() == [1, 1, 0, 2, 1, 2, 2, 0, 1, 0]
    assert set(j.fields) == {"pos", "def_grad", "mass"}
    want = _hand_made_exports(dim, [range(10)])[0]
    for f in j.fields:
        assert j.fields[f].dtype == want[f].dtype and np.array_equal(j.fields[f], want[f]), f
    assert join_slabs(_hand_made_exports(dim, per_rank), np.arange(10)).exact          # (the expected set spelled)

    j = join_slabs(_hand_made_exports(dim, [[3, 0], [], [2, 1]]))                       # one rank empty
    assert j.exact and j.counts == [2, 0, 2] and j.holder.tolist() == [0, 2, 2, 0]
    assert np.array_equal(j.fields["pos"], want["pos"][:4])

    j = join_slabs(_hand_made_exports(dim, [[7, 2, 9], [0, 8, 1], [5, 3, 6]]), np.arange(10))     # id 4 is missing
    assert not j.exact and "missing [4]" in j.problem and "duplicated []" in j.problem and "[3, 3, 3]" in j.problem
    assert not join_slabs(_hand_made_exports(dim, [[7, 2, 9], [0, 8, 1], [5, 3, 6]])).exact       # (arange(9) lacks the 9 it holds)

    j = join_slabs(_hand_made_exports(dim, [[7, 2, 9], [0, 8, 4, 1], [5, 3, 6, 8]]), np.arange(10))   # id 8 on two ranks
    assert not j.exact and "duplicated [8]" in j.problem and "missing []" in j.problem and j.counts == [3, 4, 4]

    gids = np.array([40, 10, 30, 20])                                                   # an expected set that is not arange
    j = join_slabs(_hand_made_exports(dim, [[30, 10], [40], [20]]), gids)
    assert j.exact and j.ids.tolist() == [10, 20, 30, 40] and j.holder.tolist() == [0, 2, 0, 1]
    assert np.array_equal(j.fields["mass"], np.array([10.5, 20.5, 30.5, 40.5], np.float32))
    assert not join_slabs(_hand_made_exports(dim, [[30, 10], [40], [20]])).exact

    outs = [dict(o, n0=np.array([99])) for o in _hand_made_exports(dim, per_rank)]        # a worker's saved arrays: n0 is no field
    j = join_slabs(outs, fields=("pos", "mass"))
    assert j.exact and set(j.fields) == {"pos", "mass"} and np.array_equal(j.fields["pos"], want["pos"])


def test_by_id_reorders_every_key_stably():
    from wgsparkl_amd.sharded import by_id
    out = dict(ids=np.array([5, 1, 5, 0, 1], np.uint32), pos=np.arange(10, dtype=np.float32).reshape(5, 2), slot=np.arange(5))
    got = by_id(out)
    assert set(got) == set(out)
    assert got["ids"].tolist() == [0, 1, 1, 5, 5] and got["slot"].tolist() == [3, 1, 4, 0, 2]      # equal ids keep their order
    assert np.array_equal(got["pos"], out["pos"][[3, 1, 4, 0, 2]])
    assert out["ids"].tolist() == [5, 1, 5, 0, 1]                                                  # (the export itself is left alone)


@pytest.mark.parametrize("dim,uniform", [(3, False), (3, True), (2, False)])
def test_unpack_records_reads_the_words_the_quad_table_names(dim, uniform):
    """Records synthesised from QUADS with a distinct value in every word: each key of unpack_records comes from the words the
    table names, in both dimensions and in the 3D uniform-material layout (F[8] in XM.w, the shared mass)."""
    from wgsparkl_amd.sharded import QUADS, record_floats, unpack_records
    n, nf = 5, record_floats(dim)
    rec = (1000.0 * np.arange(1, n + 1)[:, None] + np.arange(nf)[None, :]).astype(np.float32)    # word w of record i: 1000 (i + 1) + w
    rec.view(np.uint32)[:, -2] = 70 + np.arange(n)
    rec.view(np.uint32)[:, -1] = 90 + np.arange(n)
    w = lambda name, *lanes: rec[:, [4 * QUADS[dim][name] + k for k in lanes]]
    material = (0.25, 1.0, 2.0, 3.0) if uniform else None
    if dim == 3:
        want = dict(pos=w("XM", 0, 1, 2), mass=w("XM", 3)[:, 0], vel=w("CV2", 1, 2, 3),
                    affine=np.concatenate([w("CV0", 0, 1, 2, 3), w("CV1", 0, 1, 2, 3), w("CV2", 0)], 1),
                    def_grad=np.concatenate([w("F0", 0, 1, 2, 3), w("F1", 0, 1, 2, 3), w("XM", 3) if uniform else w("F2", 0)], 1),
                    cdf_normal=w("CDF0", 0, 1, 2), cdf_dist=w("CDF0", 3)[:, 0], cdf_affinity=w("CDF1", 3)[:, 0].copy().view(np.uint32))
        if uniform:
            want["mass"] = np.full(n, 0.25, np.float32)
    else:
        want = dict(pos=w("XM", 0, 1), mass=w("XM", 2)[:, 0], vel=w("CV2", 0, 1), affine=w("CV0", 0, 1, 2, 3), def_grad=w("F0", 0, 1, 2, 3),
                    cdf_normal=w("CDF0", 0, 1), cdf_dist=w("CDF0", 2)[:, 0], cdf_affinity=w("CDF0", 3)[:, 0].copy().view(np.uint32))
    want.update(ids=(70 + np.arange(n)).astype(np.uint32), cdf_stamp=(90 + np.arange(n)).astype(np.uint32))
    got = unpack_records(rec, dim, material, cdf=True)
    assert set(got) == set(want)
    for key in want:
        assert got[key].dtype == want[key].dtype and np.array_equal(got[key], want[key]), key
    plain = unpack_records(rec, dim, material)
    assert set(plain) == {"ids", "pos", "vel", "def_grad", "affine", "mass"}
    for key in plain:
        assert plain[key].dtype == got[key].dtype and np.array_equal(plain[key], got[key]), key


@pytest.mark.parametrize("dim", [3, 2])
def test_unpack_records_reads_the_plastic_quads_on_request(dim):
    """plastic=True adds dp, dp_state and phase from the words the general layout of DP0 / DP1 / DP2 names (h0..h3 | lambda, mu,
    plastic det, hardening | log_vol_gain, phase, max_stretch), with and without the cdf keys; every other key is untouched."""
    from wgsparkl_amd.sharded import QUADS, record_floats, unpack_records
    n, nf = 4, record_floats(dim)
    rec = (1000.0 * np.arange(1, n + 1)[:, None] + np.arange(nf)[None, :]).astype(np.float32)
    rec.view(np.uint32)[:, -2] = 70 + np.arange(n)
    w = lambda name, *lanes: rec[:, [4 * QUADS[dim][name] + k for k in lanes]]
    want = dict(dp=np.concatenate([w("DP0", 0, 1, 2, 3), w("DP1", 0, 1)], 1), dp_state=np.concatenate([w("DP1", 2, 3), w("DP2", 0)], 1),
                phase=w("DP2", 1, 2))
    plain = unpack_records(rec, dim)
    for cdf in (False, True):
        base = unpack_records(rec, dim, cdf=cdf)
        got = unpack_records(rec, dim, cdf=cdf, plastic=True)
        assert set(got) == set(base) | set(want)
        for key in want:
            assert got[key].dtype == np.float32 and np.array_equal(got[key], want[key]), key
        for key in base:
            assert got[key].dtype == base[key].dtype and np.array_equal(got[key], base[key]), key
    assert set(plain) == {"ids", "pos", "vel", "def_grad", "affine", "mass"}
