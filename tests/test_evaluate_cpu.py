"""genesis_amd.evaluate.evaluation on host tensors against the reference's train.evaluation
(tests/golden/evaluation_noinst.npz, recorded by tests/golden/make_golden_evaluation.py): without 'instances' no kernel runs,
the operations and their order are the reference's on the same device, so every returned float is the reference's exactly."""
import numpy as np
import pytest
import torch

from tests import evaluation_stub as S


def test_evaluation_equals_the_reference_without_instances():
    from genesis_amd.evaluate import evaluation
    g = S.load_case('noinst')
    config, iter_idx, n_eval, n_seg = S.eval_args(g)
    model, writer = S.StubModel(g), S.Writer()
    ret = evaluation(model, S.make_loader(g), writer, config, iter_idx, n_eval, n_seg)
    assert list(ret.keys()) == [str(k) for k in g['ret_keys']]
    for key, want in zip(g['ret_keys'], g['ret_vals']):
        assert isinstance(ret[str(key)], float)
        if key != 'duration':
            assert ret[str(key)] == float(want), key
    assert ret['duration'] >= 0.0
    assert [c[0] for c in writer.calls] == [str(t) for t in g['writer_tags']]
    assert [c[2] for c in writer.calls] == [int(s) for s in g['writer_steps']]
    for (tag, val, _), want in zip(writer.calls, g['writer_vals']):
        assert tag == 'val/duration' or val == float(want), tag
    assert model.training and torch.is_grad_enabled() and model.calls == int(g['num_loader_batches'])


def test_evaluation_without_a_writer_and_under_no_grad():
    from genesis_amd.evaluate import evaluation
    g = S.load_case('noinst')
    config, iter_idx, n_eval, n_seg = S.eval_args(g)
    model = S.StubModel(g)
    with torch.no_grad():
        ret = evaluation(model, S.make_loader(g), None, config, iter_idx, n_eval, n_seg)
        assert not torch.is_grad_enabled()             # the caller's mode, put back
    assert torch.is_grad_enabled() and model.training
    assert ret['err'] == float(g['ret_vals'][list(g['ret_keys']).index('err')])


def test_evaluation_restores_modes_when_forward_raises():
    from genesis_amd.evaluate import evaluation
    g = S.load_case('noinst')
    config, iter_idx, n_eval, n_seg = S.eval_args(g)
    model = S.StubModel(g, fail_at=2)
    with pytest.raises(RuntimeError, match='stub forward fails'):
        evaluation(model, S.make_loader(g), None, config, iter_idx, n_eval, n_seg)
    assert model.seen == [(False, False)] * 3                # eval mode, no grad inside the loop
    assert model.training and torch.is_grad_enabled()


def test_num_batches_rules():
    """iter_idx == 0 and config.debug stop after five batches, N_eval larger than the loader takes all of it."""
    from genesis_amd.evaluate import evaluation
    from genesis_amd.compat.attrdict import AttrDict
    g = S.load_case('noinst')
    for config, iter_idx, n_eval, want in ((AttrDict(debug=False, gpu=False), 0, None, 5),
                                           (AttrDict(debug=True, gpu=False), 3, None, 5),
                                           (AttrDict(debug=False, gpu=False), 3, 8, 2),
                                           (AttrDict(debug=False, gpu=False), 3, 1000, 6)):
        model = S.StubModel(g)
        ret = evaluation(model, S.make_loader(g), None, config, iter_idx, n_eval)
        assert ret['num_batches'] == want and model.calls == want
        err = torch.from_numpy(g['loss/err'])[:want]
        assert ret['err'] == float(sum(e.mean(0) for e in err) / want)
        np.testing.assert_allclose(ret['err_element'], ret['err'] / (3 * 16 * 16), rtol=1e-6)
