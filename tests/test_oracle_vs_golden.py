"""Pins the oracle (oracle/v2_oracle.py) against golden vectors captured from the real
reference, and against the reference's own model: the live import when the reference tree is present, its recording otherwise."""
import numpy as np
import pytest
import torch

from genesis_amd import testing as T
from oracle import v2_oracle as O
from oracle import ref_import as R
from tests.common import ALL_CASES, DYN_CASES, SAMPLE_CASES, Golden, SampleGolden, load_live_recording


def _params(gold, requires_grad=False):
    tmpl = O.template_state_dict(gold.cfg)
    sd = gold.weights(tmpl)
    return {k: v.clone().requires_grad_(requires_grad) for k, v in sd.items()}


@pytest.mark.parametrize('case', ALL_CASES + DYN_CASES)
@pytest.mark.parametrize('reference_form', [True, False])
def test_forward_and_grads(case, reference_form):
    if case == 'cfg5' and reference_form:
        pytest.skip('128x128 K=11 reference-form covered by the deduplicated form')
    gold = Golden(case)
    p = _params(gold, True)
    x, rand_pixel, eps_k = gold.inputs()
    recon, losses, stats, att, comp = O.v2_forward(
        p, x, gold.cfg, rand_pixel, eps_k, reference_form=reference_form)
    gold.check_forward(recon, losses, stats, att, comp, rtol=2e-5, atol=2e-6)
    err, kl_l, kl_m = O.aggregate_losses(losses)
    assert abs(float(err) - float(gold.g['loss/err'])) <= 1e-5 * abs(float(err))
    (err + kl_l + kl_m).backward()
    grads = [(k, v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in p.items()]
    gold.check_grads(grads)


@pytest.mark.parametrize('case', ['tiny', 'tiny_klm', 'metric'])
def test_train_steps(case):
    gold = Golden(case)
    p = _params(gold, True)
    x, _, _ = gold.inputs()
    geco = O.make_geco(gold.S)
    opt = torch.optim.Adam(list(p.values()), 1e-4)
    hist = gold.g['train_hist']
    for it in range(3):
        rp, eps = gold.noise(1 + it)
        elbo, err, kl, beta = O.train_step(p, opt, geco, x, gold.cfg, rp, eps)
        np.testing.assert_allclose([elbo, err, kl, beta], hist[it, :4], rtol=1e-3)
        assert abs(elbo - hist[it, 0]) <= 1e-3 * abs(hist[it, 0])  # north_star ELBO bound
    assert abs(float(geco.beta) - float(gold.g['train_beta_final'])) <= 1e-5


def test_masks_sum_to_one():
    """The one numerical invariant the reference itself pins: utils/misc.py:258-270."""
    gold = Golden('tiny')
    p = _params(gold)
    x, rp, eps = gold.inputs()
    _, _, stats, _, _ = O.v2_forward(p, x, gold.cfg, rp, eps)
    for key in ('log_m_k', 'log_m_r_k'):
        s = torch.stack(stats[key], 4).exp().sum(4)
        assert float((s - 1).abs().max()) < 1e-3


@pytest.mark.parametrize('case', SAMPLE_CASES)
def test_sample_vs_golden(case):
    """GenesisV2.sample (models/genesisv2_config.py:227-256): the oracle's rollout + decode on the reference's recorded
    draws against the reference's own outputs."""
    gold = SampleGolden(case)
    tmpl = O.template_state_dict(gold.cfg)
    from genesis_amd import testing as T
    p = T.formula_state_dict(tmpl)
    recon, x_k, log_m_k, z_k = O.v2_sample(p, gold.cfg, list(gold.eps.unbind(0)))
    gold.check_all(recon, x_k, log_m_k, z_k, rtol=2e-5, atol=2e-6,
                   mx_k=[x * m.exp() for x, m in zip(x_k, log_m_k)])


LIVE_CFG = dict(K_steps=5, img_size=32, feat_dim=16)


def live_weights(sd):
    """The weights both sides run on: closed-form (genesis_amd.testing.formula_state_dict, the golden fixtures' weights, a
    function of the names, shapes and dtypes of `sd`), colour-head gate 0.4."""
    w = T.formula_state_dict(sd)
    w['att_process.colour_head.gate.gate'] = torch.tensor(0.4, dtype=sd['att_process.colour_head.gate.gate'].dtype)
    return w


def live_reference_run(mods):
    """The reference's own model (initialised under seed 3) -- its state_dict is returned as it initialised it --, run on
    live_weights on x ~ U[0, 1), forward under noise seed 5: (state_dict, x, outputs).  Recorded for machines without the
    reference by tests/golden/make_golden_live.py."""
    torch.manual_seed(3)
    model = mods['genesisv2_config'].load(R.reference_cfg(**O.make_cfg(**LIVE_CFG)))
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    model.load_state_dict(live_weights(sd))
    x = torch.rand(3, 3, 32, 32)
    torch.manual_seed(5)
    r_recon, r_losses, r_stats, _, r_comp = model(x)
    return sd, x, {'recon': r_recon, 'err': r_losses['err'], 'kl_l_k': torch.stack(r_losses['kl_l_k']),
                   'z_k': torch.stack(r_comp['z_k'])}


def test_live_against_reference_import():
    """The oracle against the reference's own model and forward: imported live when the reference tree is present, else
    that same run as recorded from the import (tests/golden/live_v2.npz)."""
    if R.reference_available():
        sd, x, r = live_reference_run(R.import_reference())
    else:
        sd, x, r = load_live_recording('v2')
    cfgd = O.make_cfg(**LIVE_CFG)
    assert list(sd.keys()) == list(O.param_shapes(cfgd).keys())
    for k, (shape, dt) in O.param_shapes(cfgd).items():
        assert tuple(sd[k].shape) == tuple(shape) and sd[k].dtype == dt, k
    assert torch.equal(sd['att_process.log_sigma'], O.default_log_sigma(cfgd).double())
    torch.manual_seed(5)  # oracle draws its own noise in the same order
    recon, losses, stats, _, comp = O.v2_forward(live_weights(sd), x, cfgd)
    assert torch.allclose(recon, r['recon'], rtol=1e-5, atol=1e-6)
    assert torch.allclose(losses['err'], r['err'], rtol=1e-6)
    for a, b in zip(losses['kl_l_k'], r['kl_l_k']):
        assert torch.allclose(a, b, rtol=1e-5, atol=1e-5)
    assert len(comp['z_k']) == len(r['z_k'])
    for a, b in zip(comp['z_k'], r['z_k']):
        assert torch.allclose(a, b, rtol=1e-5, atol=1e-6)
