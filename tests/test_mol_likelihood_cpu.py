"""CPU: the per-molecule likelihood fixtures are consistent with themselves, the draw key of the latent normals has the
properties ``log_likelihood`` promises (numpy restatement, tests/likelihood_oracle.py), and bad arguments are refused before
anything reaches a device."""
import numpy as np
import pytest
import torch

import likelihood_oracle as LO
import mol_likelihood_fixtures as LF
import sample_oracle as SO

SEED = 0x5EED0123456789AB


def test_there_is_one_fixture_per_decoder_and_cell():
    got = sorted((LF.LLGolden(n).decoder, LF.LLGolden(n).rnn) for n in LF.names())
    assert got == [("hier", "GRU"), ("hier", "LSTM"), ("motif", "GRU"), ("motif", "LSTM")]
    assert {kind for _, kind in LF.cases()} == {"hier-prop", "hier-prop-opt", "prop", "prop-opt"}


@pytest.mark.parametrize("name", LF.names())
def test_fixture_is_self_consistent(name):
    g = LF.LLGolden(name)
    z = g.z
    K, B, L = g.K, g.B, g.latent
    assert K == 3 and z["eps"].shape == (K, B, L) and z["parts"].shape == (K, B, 4)
    assert z["eps"].dtype == np.float32 and z["mean"].dtype == np.float32 and z["pre_var"].dtype == np.float32
    # the parts add up to the reference's own batch loss x B (an fp32 sum of the same rows)
    for k in range(K):
        want = z["ref_loss"][k] * B
        assert abs(z["parts"][k].sum() - want) <= 1e-5 * abs(want), (k, z["parts"][k].sum(), want)
    assert (z["parts"] >= 0).all()
    # a molecule with attachment predictions and one without; two molecules whose largest cluster differs
    has = (z["parts"][:, :, 3] > 0).any(axis=0)
    assert has.any() and not has.all()
    assert len(set(z["largest_cluster"].tolist())) > 1
    specs = g.specs()
    assert [max(len(c) for c in m.clusters) for m in specs] == z["largest_cluster"].tolist()
    assert int(z["ref_max_cls_size"]) == 2 * max(z["largest_cluster"])
    # kl, elbo, iwae are the fp64 formulas on the recorded mean / pre_var / eps / parts
    _, kl, logpq = LO.latent_terms(z["mean"], z["pre_var"], z["eps"])
    elbo, iwae = LO.iwae_finish(z["parts"], logpq, kl)
    for a, b in ((kl, z["kl"]), (logpq, z["logpq"]), (elbo, z["elbo"]), (iwae, z["iwae"])):
        assert np.allclose(a, b, rtol=1e-12, atol=1e-12)
    assert (kl > 0).all()
    assert (iwae <= 0).all() and (elbo <= 0).all()


def test_k1_iwae_is_the_single_sample_elbo_estimate():
    rs = np.random.RandomState(3)
    parts, logpq, kl = rs.rand(1, 5, 4) * 7, rs.randn(1, 5), rs.rand(5)
    _, iwae = LO.iwae_finish(parts, logpq, kl)
    assert np.allclose(iwae, -parts.sum(axis=2)[0] + logpq[0], rtol=1e-14)


def test_draw_key_prefix_property():
    """the first K draws of a K' > K call are the K call's"""
    ids = np.array([0, 7, 1 << 31, 12345])
    small, large = LO.latent_normals(SEED, ids, 3, 8), LO.latent_normals(SEED, ids, 65, 8)
    assert np.array_equal(large[:3], small)
    assert not np.array_equal(large[3:6], small)


def test_draw_key_batch_independence():
    """a molecule's draws follow its sample id: not its place in the batch, not the batch size"""
    ids = np.array([5, 900, 33, 2, 77])
    full = LO.latent_normals(SEED, ids, 4, 24)
    perm = np.array([3, 0, 4, 1, 2])
    assert np.array_equal(LO.latent_normals(SEED, ids[perm], 4, 24), full[:, perm])
    assert np.array_equal(LO.latent_normals(SEED, ids[[2]], 4, 24), full[:, [2]])
    assert not np.array_equal(LO.latent_normals(SEED + 1, ids, 4, 24), full)


def test_draw_key_is_the_stream_at_its_own_site():
    """counter k * L + column at site LATENT: the words of tests/sample_oracle.py, not the prior's"""
    assert LO.SITE_LATENT not in (SO.SITE_TOPO, SO.SITE_BEAM, SO.SITE_PRIOR)
    K, L, ids = 3, 8, np.array([4, 9])
    eps = LO.latent_normals(SEED, ids, K, L)
    for k in range(K):
        for c in range(L):
            m0 = SO.words(SEED, LO.SITE_LATENT, ids, k * L + c, 0).astype(np.float64)
            m1 = SO.words(SEED, LO.SITE_LATENT, ids, k * L + c, 1).astype(np.float64)
            want = np.sqrt(-2 * np.log((m0 + 1) * 2.0 ** -24)) * np.cos(np.pi * (2 * m1 * 2.0 ** -24))
            assert np.array_equal(eps[k, :, c], want)
    # K = 1 at the prior's site would be sample_normal's rows: the sites differ, so the values do
    assert not np.array_equal(eps[0], SO.normals(SEED, ids, L))


def test_draw_moments():
    z = LO.latent_normals(SEED, np.arange(512), 16, 32).reshape(-1)
    assert abs(z.mean()) <= 5 / np.sqrt(z.size) and abs(z.var() - 1) <= 5 * np.sqrt(2.0 / z.size)


# ---------------------------------------------------------------------------------------------- argument errors
@pytest.fixture(scope="module")
def hier():
    g = LF.LLGolden("ll_hier_gru_s40")
    batch, sch = g.batch()
    return g, g.model("hier-prop"), batch, sch


def test_bad_arguments_raise_before_any_launch(hier):
    """the model sits on the CPU, where no launch can succeed: every error below comes from the argument checks"""
    g, model, batch, sch = hier
    B, L = g.B, g.latent
    ll = lambda **kw: model.log_likelihood(batch, schedule=sch, **kw)
    for K in (0, -1, 1025, 2.5):
        with pytest.raises(ValueError, match="n_samples"):
            ll(n_samples=K)
    good = torch.zeros(3, B, L)
    for eps, K in ((good, 2), (good[:, :, :-1], 3), (good[:, :-1], 3), (good[0], 3)):        # shape / n_samples disagree
        with pytest.raises(ValueError, match="eps of shape"):
            ll(n_samples=K, eps=eps)
    with pytest.raises(ValueError, match="float32"):
        ll(n_samples=3, eps=good.double())
    with pytest.raises(ValueError, match="float32 tensor on"):
        ll(n_samples=3, eps=good.to("meta"))
    with pytest.raises(ValueError, match="float32"):
        ll(n_samples=3, eps=good.numpy())
    with pytest.raises(ValueError, match="sample_ids"):
        ll(n_samples=2, sample_ids=list(range(B + 1)))
    with pytest.raises(ValueError, match="no graphs"):
        model.log_likelihood(batch)                   # (the fixture's batch carries no graphs: a schedule must come with it)
    assert sch.max_cls_size == int(g.z["ref_max_cls_size"])
    with pytest.raises(ValueError, match="max_cls_size"):
        ll(max_cls_size=sch.max_cls_size - 1)


def test_training_mode_with_dropout_raises():
    g = LF.LLGolden("ll_motif_gru_s60")
    batch, sch = g.batch()
    model = g.model("prop", dropout=0.1)
    model.train()
    with pytest.raises(NotImplementedError, match=r"PropertyVAE\.log_likelihood runs without dropout: call model\.eval\(\) first"):
        model.log_likelihood(batch, schedule=sch)
