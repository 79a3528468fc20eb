"""genesis_amd.evaluate on the device: the instance-bearing recordings of the reference's train.evaluation and
utils.misc.dataset_ari (tests/golden/evaluation_*.npz, tests/evaluation_stub.py), and one real GENESIS-V2 model against a loop
written with the existing average_ari / average_segcover.  Segmentation keys: the tolerances of tests/test_metrics.py (ARI
1e-12, covering 2e-7 relative).  Loss keys: exactly the same torch expressions evaluated on the device by the test
(tests/test_evaluate_cpu.py pins them to the reference)."""
import numpy as np
import pytest
import torch

from tests import evaluation_stub as S

pytestmark = pytest.mark.gpu
ARI = dict(rtol=1e-12, atol=1e-12)
COVER = dict(rtol=2e-7)


def tol(key):
    return ARI if 'ari' in key else COVER


def loss_expectations(g, num_batches):
    """train.py:515-532, 567, 571 on the device: per key sum(batch means) / len, 'elbo', 'err_element'."""
    dev = 'cuda'
    keys = [str(k) for k in g['loss_keys']]
    L = {k: torch.from_numpy(g['loss/' + k]).to(dev) for k in keys}
    per = {k: [] for k in keys + ['elbo']}
    for i in range(num_batches):
        m = {k: (torch.stack(list(L[k][i].unbind(0)), 1).sum(1).mean(0) if k in S.LIST_LOSSES else L[k][i].mean(0)) for k in keys}
        for k in keys:
            per[k].append(m[k])
        kl_m = m['kl_m_k'] if 'kl_m_k' in m else m.get('kl_m', torch.tensor(0))
        kl_l = m['kl_l_k'] if 'kl_l_k' in m else m.get('kl_l', torch.tensor(0))
        per['elbo'].append(m['err'] + kl_m + kl_l)
    mean = {k: sum(v) / len(v) for k, v in per.items()}
    out = {k: float(v) for k, v in mean.items()}
    out['err_element'] = float(mean['err'] / int(np.prod(g['input_shape'][1:4])))
    return out


@pytest.mark.parametrize('case', S.INSTANCE_CASES)
@pytest.mark.parametrize('packed', [False, True])
def test_evaluation_against_the_reference_recording(case, packed):
    from genesis_amd.evaluate import evaluation
    g = S.load_case(case)
    config, iter_idx, n_eval, n_seg = S.eval_args(g)
    if packed:
        model, loader = S.StubModel(g, 'cuda', packed=True), S.make_loader(g, 'cuda')
    else:                               # host batches, moved by evaluation() as the reference does under config.gpu
        model, loader, config = S.StubModel(g, 'cuda'), S.make_loader(g), type(config)(debug=False, gpu=True)
    writer = S.Writer()
    ret = evaluation(model, loader, writer, config, iter_idx, n_eval, n_seg)
    keys = [str(k) for k in g['ret_keys']]
    assert list(ret.keys()) == keys
    want = dict(zip(keys, g['ret_vals']))
    losses = loss_expectations(g, int(want['num_batches']))
    for key in keys:
        if 'ari' in key or 'msc' in key:
            np.testing.assert_allclose(ret[key], want[key], err_msg=key, **tol(key))
        elif key in losses:
            assert ret[key] == losses[key], key
    assert ret['num_batches'] == want['num_batches']
    assert [c[0] for c in writer.calls] == ['val/' + k for k in keys]
    assert [c[1] for c in writer.calls] == [ret[k] for k in keys] and {c[2] for c in writer.calls} == {iter_idx}
    assert model.training and torch.is_grad_enabled()
    if not packed:
        assert all(v.is_cuda for b in loader[:int(want['num_batches'])] for v in b.values())


@pytest.mark.parametrize('case', S.INSTANCE_CASES)
def test_dataset_ari_and_seg_metrics_from_model(case):
    from genesis_amd.evaluate import dataset_ari, seg_metrics_from_model
    g = S.load_case(case)
    model = S.StubModel(g, 'cuda', packed=True)
    avg, avg_fg, lst, lst_fg = dataset_ari(model, S.make_loader(g), int(g['num_images']))
    np.testing.assert_allclose(avg, float(g['dari_avg']), **ARI)
    np.testing.assert_allclose(avg_fg, float(g['dari_avg_fg']), **ARI)
    np.testing.assert_allclose(lst, g['dari_list'], **ARI)              # the last batch's lists, as the reference returns
    np.testing.assert_allclose(lst_fg, g['dari_list_fg'], **ARI)
    assert model.training and model.calls == 3 and isinstance(avg, float) and isinstance(lst, list)
    out = seg_metrics_from_model(S.StubModel(g, 'cuda'), S.make_loader(g))
    assert set(out) == {k[3:] for k in g.files if k.startswith('sm_')}
    for key, val in out.items():
        np.testing.assert_allclose(val, float(g['sm_' + key]), err_msg=key, **tol(key))


def test_dataset_ari_returns_zeros_without_labels_or_masks():
    from genesis_amd.evaluate import dataset_ari
    g = S.load_case('noinst')
    assert dataset_ari(S.StubModel(g, 'cuda'), S.make_loader(g)) == (0., 0., [0], [0])
    g = S.load_case('all')
    model = S.StubModel(g, 'cuda')
    model.masks.pop('log_m_k')
    assert dataset_ari(model, S.make_loader(g)) == (0., 0., [0], [0])


def test_real_model_against_a_loop_of_the_existing_functions():
    """GENESIS-V2, B = 2, K = 3, 32 x 32, closed-form weights: evaluation() and seg_metrics_from_model() against the
    reference's loop with this package's average_ari / average_segcover in it; both mask fields are present."""
    import genesis_amd.genesisv2_config as G
    from genesis_amd import metrics as M
    from genesis_amd import testing as T
    from genesis_amd.compat.attrdict import AttrDict
    from genesis_amd.evaluate import evaluation, seg_metrics_from_model
    from oracle import v2_oracle as O
    cfg = O.make_cfg(K_steps=3, img_size=32, feat_dim=16)
    torch.manual_seed(0)
    model = G.load(AttrDict(dict(cfg, debug=False, multi_gpu=False)))
    model.load_state_dict(T.formula_state_dict(model.state_dict()))
    model = model.to('cuda').train()
    gen = torch.Generator().manual_seed(3)
    batches = [{'input': T.make_input(7 + i, 2, 32).cuda(),
                'instances': torch.randint(0, 4, (2, 1, 8, 8), generator=gen).repeat_interleave(4, 2).repeat_interleave(4, 3).cuda()}
               for i in range(3)]

    torch.manual_seed(11)
    ret = evaluation(model, S.Loader(batches, 2), None, AttrDict(debug=False, gpu=True), 1, None, N_seg_metrics=5)
    assert model.training and torch.is_grad_enabled()
    torch.manual_seed(11)
    sm = seg_metrics_from_model(model, batches)
    model.train()

    torch.manual_seed(11)
    model.eval()
    lists = {}
    with torch.no_grad():
        for b in batches:
            _, losses, stats, _, _ = model(b['input'])
            lists.setdefault('err', []).append(losses.err.mean(0))
            lists.setdefault('kl_l_k', []).append(torch.stack(losses.kl_l_k, 1).sum(1).mean(0))
            for mode, r in (('log_m_k', ''), ('log_m_r_k', '_r')):
                ins_seg = torch.argmax(torch.cat(stats[mode], 1), 1, True)
                lists.setdefault('ari' + r, []).append(M.average_ari(stats[mode], b['instances'])[0])
                lists.setdefault('ari_fg' + r, []).append(M.average_ari(stats[mode], b['instances'], True)[0])
                lists.setdefault('msc' + r, []).append(M.average_segcover(b['instances'], ins_seg)[0])
                lists.setdefault('msc_fg' + r, []).append(M.average_segcover(b['instances'], ins_seg, True)[0])
    model.train()
    want = {k: float(sum(v) / len(v)) for k, v in lists.items()}
    assert ret['num_batches'] == 3.0
    for key, val in want.items():
        if 'ari' in key or 'msc' in key:
            np.testing.assert_allclose(ret[key], val, err_msg=key, **tol(key))
        else:
            assert ret[key] == val, key
    for key in ('ari_fg', 'msc_fg', 'ari_fg_r', 'msc_fg_r'):
        np.testing.assert_allclose(sm[key], want[key], err_msg=key, **tol(key))
