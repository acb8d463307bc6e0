"""CPU: the property heads / latent search feature without a GPU -- module layout against the reference's (state_dict
keys as stored in the fixtures), the numpy restatement (tests/property_oracle.py) against the reference's own outputs, the
library's new entry points, and the max_steps / capped contract."""
import numpy as np
import pytest
import torch

import property_fixtures as pf
import property_oracle as po


def _vocab(g):
    from ggpm_amd.vocab import IndexPairVocab
    return IndexPairVocab(g.n_motif, g.n_attach)


@pytest.mark.parametrize("name", pf.names("propopt"))
def test_hierpropoptvae_state_dict_keys_are_the_references(name):
    from ggpm_amd.property_vae import HierPropOptVAE
    g = pf.PropOptGolden(name)
    model = HierPropOptVAE(g.args(_vocab(g)))
    # (as a set: the decoder registers its sub-modules in its own order, as HierPropertyVAE's does)
    assert sorted(model.state_dict().keys()) == sorted(str(k) for k in g.z["state_keys"])
    assert sorted(k for k, _ in model.named_parameters()) == sorted(str(k) for k in g.z["param_names"])
    # the sub-modules themselves come in the reference's order
    assert list(dict.fromkeys(k.split(".")[0] for k in model.state_dict())) == \
        list(dict.fromkeys(str(k).split(".")[0] for k in g.z["state_keys"]))
    if g.scaling:
        assert all(p.dtype == torch.float64 for p in model.loss_weigh.parameters())


@pytest.mark.parametrize("name", pf.names("propsearch"))
def test_property_optimizer_state_dict_keys_are_the_references(name):
    from ggpm_amd.property import PropertyOptimizer
    z = pf.load(name)
    lh = [int(v) for v in z["linear_hidden"]]
    opt = PropertyOptimizer(int(z["latent"]) // 2, lh[0] if len(lh) == 1 else lh, 0.1)
    assert list(opt.state_dict().keys()) == [str(k) for k in z["state_keys"]]


def test_odd_latent_size_is_a_clear_error():
    from ggpm_amd.property_vae import HierPropOptVAE
    g = pf.PropOptGolden(pf.names("propopt")[0])
    a = g.args(_vocab(g))
    a.latent_size = 7
    with pytest.raises(ValueError, match="even"):
        HierPropOptVAE(a)


def _search_case(name, dtype=np.float64):
    z = pf.load(name)
    sd = {k[2:]: z[k] for k in z.files if k.startswith("w/")}
    patience, thr, delta, lr = [float(v) for v in z["params"]]
    homo, lumo = po.head_layers(sd, "homo_linear"), po.head_layers(sd, "lumo_linear")
    half = int(z["latent"]) // 2
    args = (str(z["mode"]), homo, lumo, z["z"], half, z["t_homo"], z["t_lumo"], lr, int(z["steps"]), delta, patience, thr)
    return z, args


@pytest.mark.parametrize("name", pf.names("propsearch"))
def test_search_restatement_reproduces_the_reference(name):
    """fp64: the reference's fp64 run (decisions exactly, latents to 1e-9); fp32: the step counts of its fp32 run."""
    z, args = _search_case(name)
    marg = po.Margins()
    z64, p64, n64, st = po.search(*args, 10000, np.float64, marg)
    assert (st == po.DONE).all()
    assert (n64 == z["steps_ref"]).all()
    assert np.abs(z64 - z["z_ref64"]).max() <= 1e-9 * max(1.0, np.abs(z64).max())
    assert np.abs(np.stack(p64) - z["pred_ref64"]).max() <= 1e-9 * max(1.0, np.abs(z["pred_ref64"]).max())
    assert marg.min >= 1e-3 and abs(marg.min - float(z["min_margin"])) <= 1e-9
    z32, p32, n32, _ = po.search(*args, 10000, np.float32)
    assert (n32 == z["steps_ref"]).all()
    # the calibrated bound the GPU test applies, met here by a second fp32 summation order
    bound = np.maximum(1e-4, 4 * np.abs(z["z_ref"].astype(np.float64) - z["z_ref64"]))
    assert (np.abs(z32 - z["z_ref"]) <= bound).all()


@pytest.mark.parametrize("name", pf.names("propopt"))
def test_heads_restatement_reproduces_the_reference_fine_tune_step(name):
    """The heads part of the reference's HierPropOptVAE step: HOMO / LUMO MSE (before loss scaling) and every gradient of
    property_optim, from the latent the reference's forward produced."""
    g = pf.PropOptGolden(name)
    sd = {k[len("property_optim."):]: v for k, v in g.state_dict().items() if k.startswith("property_optim.")}
    homo, lumo = po.head_layers(sd, "homo_linear"), po.head_layers(sd, "lumo_linear")
    half = g.latent // 2
    dloss = (1.0, 1.0)
    if g.scaling:
        lw = g.state_dict()
        dloss = (float(np.exp(-lw["loss_weigh.homo_log_var"][0])), float(np.exp(-lw["loss_weigh.lumo_log_var"][0])))
    out = po.heads_step(homo, lumo, g.z["latent"].astype(np.float64), half, g.z["t_homo"].astype(np.float64),
                        g.z["t_lumo"].astype(np.float64), dloss=dloss)
    m = g.metrics()
    if not g.scaling:
        assert abs(out["loss"][0] - m["HOMO_MSE"]) <= 1e-5 * max(1, m["HOMO_MSE"])
        assert abs(out["loss"][1] - m["LUMO_MSE"]) <= 1e-5 * max(1, m["LUMO_MSE"])
    for hi, head in enumerate(("homo_linear", "lumo_linear")):
        for i, (dW, db) in enumerate(out["grads"][hi]):
            for suffix, got in (("weight", dW), ("bias", db)):
                want = g.z["grad/property_optim.%s.linear.%d.%s" % (head, 3 * i, suffix)].astype(np.float64)
                assert np.abs(got - want).max() <= 1e-5 * max(1e-3, np.abs(want).max()), (head, i, suffix)


def test_restatement_caps_a_search_that_would_never_end():
    """Loss exactly 0 -> |0 - 0| / 0 is NaN -> the patience resets on every body: the reference loops forever; the
    contract ends the molecule after max_steps bodies with status capped.  Fixed mode with steps > max_steps is capped
    too."""
    rs = np.random.RandomState(3)
    half = 6
    homo = [(rs.standard_normal((8, half)), rs.standard_normal(8)), (np.zeros((1, 8)), np.array([0.25]))]
    lumo = [(rs.standard_normal((8, half)), rs.standard_normal(8)), (np.zeros((1, 8)), np.array([-0.5]))]
    z = rs.standard_normal((3, 2 * half))
    t_h, t_l = np.full(3, 0.25), np.full(3, -0.5)
    for mode in ("patience", "soft"):
        delta = -1.0        # soft: a negative delta never stops it either
        zo, preds, n, st = po.search(mode, homo, lumo, z, half, t_h, t_l, 1.0, 20, delta, 5, 0.1, 50, np.float32)
        assert (n == 50).all() and (st == po.CAPPED).all()
        assert np.allclose(zo, z.astype(np.float32))          # zero gradient: the latent never moves
    _, _, n, st = po.search("fixed", homo, lumo, z, half, t_h, t_l, 1.0, 20, 0.1, 5, 0.1, 7)
    assert (n == 7).all() and (st == po.CAPPED).all()
    _, _, n, st = po.search("fixed", homo, lumo, z, half, t_h, t_l, 1.0, 7, 0.1, 5, 0.1, 7)
    assert (n == 7).all() and (st == po.DONE).all()


def test_library_exports_the_property_entry_points():
    from ggpm_amd import _lib, build
    build.build(verbose=False)
    lib = _lib.load()
    for name in ("ggpm_property_heads_workspace_bytes", "ggpm_property_heads_forward", "ggpm_property_heads_backward",
                 "ggpm_property_latent_search"):
        assert hasattr(lib, name), name
    # the workspace query is host-only: heads of 12 -> 64 -> 64 -> 1 over 20 rows
    from ggpm_amd.property import PropertyOptimizer
    import ctypes
    opt = PropertyOptimizer(12, [64, 64], 0.1)
    h, l = opt.homo_linear.c_struct(), opt.lumo_linear.c_struct()
    per_head = (2 * 20 * 64 + 2 * 20 * 64)          # stashed inputs of Linear 1, 2; the backward's ping-pong
    assert lib.ggpm_property_heads_workspace_bytes(20, 12, ctypes.byref(h), ctypes.byref(l)) >= 2 * per_head * 4
    assert lib.ggpm_property_heads_workspace_bytes(20, 11, ctypes.byref(h), ctypes.byref(l)) == 0     # width mismatch


def test_header_structs_match_the_ctypes_mirrors(tmp_path):
    """ggpm_prop_head / ggpm_prop_head_grads: sizeof and field offsets from a C program against include/ggpm_hip.h."""
    import os
    import subprocess
    from ggpm_amd.property import PropHeadC, PropHeadGradsC
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lines = []
    for cname, cls in (("ggpm_prop_head", PropHeadC), ("ggpm_prop_head_grads", PropHeadGradsC)):
        lines.append('printf("%%zu", sizeof(%s));' % cname)
        for f, _ in cls._fields_:
            lines.append('printf(" %%zu", offsetof(%s, %s));' % (cname, f))
        lines.append('printf("\\n");')
    src = tmp_path / "abi.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ggpm_hip.h"\nint main(void) {\n%s\nreturn 0; }\n'
                   % "\n".join(lines))
    exe = tmp_path / "abi"
    subprocess.check_call(["cc", "-I", os.path.join(root, "include"), str(src), "-o", str(exe)])
    got = subprocess.check_output([str(exe)]).decode().split("\n")
    for line, cls in zip(got, (PropHeadC, PropHeadGradsC)):
        want = [ctypes_size(cls)] + [getattr(cls, f).offset for f, _ in cls._fields_]
        assert [int(v) for v in line.split()] == want, cls.__name__


def ctypes_size(cls):
    import ctypes
    return ctypes.sizeof(cls)
