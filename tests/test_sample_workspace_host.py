"""Host: the reverse loop's workspace sizes (ldm_sample_workspace_floats) and zero-filled ranges
(ldm_sample_workspace_zeroed) over a grid of configurations, against the numbers recorded in
tests/golden/sample_workspace_sizes.json before the workspace's tail was stated once (carve_sample, csrc/unet.hip).
Both functions read only fields of their arguments: no device is needed and no pointer is dereferenced."""
import ctypes
import json
import os

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sample_workspace_sizes.json")


def filled_weights(L):
    """An ldm_unet_weights with everything the size functions read set: the folded loop on the step kernels with the
    bottleneck's value fold, and split-K workspaces in the plans (the K/V projections' the largest)."""
    w = L.UNetWeights()
    w.use_fold, w.use_step, w.step_bneck_w = 1, 2, 4096
    for i in range(9):
        w.conv_plan[i].ws_floats = 1000 + 37 * i
    for j in range(2):
        w.ca_plan_q[j].ws_floats, w.ca_plan_kv[j].ws_floats, w.ca_plan_o[j].ws_floats = 501 + j, 4099 + 64 * j, 77
    return w


def grid_values(lib, L):
    """{case name: [floats, zeroed ranges x 4]} over the grid."""
    byref = ctypes.byref
    out = {}
    for wname, w in (("null", None), ("filled", filled_weights(L))):
        for B in (1, 2, 3, 8):
            for H, W in ((8, 8), (16, 64), (16, 128)):
                own = ((H // 4) * (W // 4), (H // 8) * (W // 8))
                for nsteps in (0, 1, 10):
                    for keys in ((0, 0), own, (2 * own[0], 2 * own[1])):
                        for guided in (0, 1):
                            for keep in (0, 1):
                                shape = L.UNetShape(B, 32, H, W, 64)
                                # (a set flag stands for an option's pointers: only whether they are set is read)
                                a = L.SampleArgs(nsteps=nsteps, S5=keys[0], S6=keys[1], s5_base=guided, s6_base=guided,
                                                 guide_scale=guided, z0=keep, n0=keep, keep=keep, keep_coef=keep)
                                wp = byref(w) if w is not None else None
                                n = lib.ldm_sample_workspace_floats(byref(shape), wp, byref(a))
                                r = (ctypes.c_int64 * 4)()
                                rc = lib.ldm_sample_workspace_zeroed(byref(shape), wp, byref(a), r)
                                assert rc == 0
                                out[f"{wname}/B{B}/{H}x{W}/n{nsteps}/S{keys[0]},{keys[1]}/g{guided}/k{keep}"] = \
                                    [int(n)] + [int(v) for v in r]
    return out


def test_workspace_sizes_are_the_recorded_ones():
    from ldm_amd import _lib as L
    with open(GOLDEN) as f:
        want = json.load(f)
    got = grid_values(L.load(), L)
    assert len(want) == 2 * 4 * 3 * 3 * 3 * 2 * 2 and set(got) == set(want)
    bad = [k for k in want if got[k] != want[k]]
    assert not bad, f"{len(bad)} configurations changed size, e.g. {bad[0]}: {got[bad[0]]} != {want[bad[0]]}"
    assert all(v[0] > 0 for v in got.values())
    # the keep and the guidance each enlarge the workspace, and every step adds its time embeddings
    k = "filled/B2/16x64/n10/S0,0/"
    assert got[k + "g0/k1"][0] > got[k + "g0/k0"][0] and got[k + "g1/k0"][0] > got[k + "g0/k0"][0]
    assert got[k + "g0/k0"][0] - got[k.replace("n10", "n0") + "g0/k0"][0] == 10 * 2 * 128
