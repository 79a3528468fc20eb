"""genesis_amd.visualise on the device (gx_vis_compose): make_grid, colour_seg_masks, the argmax and exp kinds, visualise_outputs
against what the reference's own function handed to its writer (tests/golden/visualise_*.npz), one run on a real model, the
sheets and their PNGs.  Bit-exact everywhere but the exponentials, which may differ from the correctly rounded value by 1 ulp:
the device math library's documented bound for expf."""
import numpy as np
import pytest
import torch

from genesis_amd import visualise as vis
from genesis_amd._lib import GenesisHipError
from genesis_amd.compat.attrdict import AttrDict
from oracle import ref_import as R
from tests import vis_restatement as V
from tests import visualise_stub as S

pytestmark = pytest.mark.gpu
DEV = 'cuda'
PALETTE32 = [[(7 * i + 1) % 256, (13 * i + 2) % 256, 255 - i] for i in range(32)]


def _ulps(a, b):
    """Distance in units in the last place between two fp32 arrays of non-negative values."""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    assert a.shape == b.shape
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


def _exp32(x):
    """The fp64 exponential rounded to fp32."""
    with np.errstate(under='ignore'):
        return np.exp(np.asarray(x, np.float64)).astype(np.float32)


def _values(n, C, H, W, seed):
    return torch.from_numpy(np.random.RandomState(seed).rand(n, C, H, W).astype(np.float32))


# ---- make_grid -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('H, W', [(5, 7), (8, 8), (1, 1)])
def test_make_grid_matches_the_restatement(H, W):
    for n in (1, 3, 8, 11):
        for C in (1, 3):
            x = _values(n, C, H, W, 100 * n + C)
            for nrow, padding in ((8, 2), (4, 2), (8, 0), (4, 0)):
                got = vis.make_grid(x.to(DEV), nrow=nrow, padding=padding, pad_value=0.5)
                want = V.make_grid(x.numpy(), nrow, padding, 0.5)
                assert got.is_cuda and got.dtype == torch.float32 and tuple(got.shape) == want.shape, (n, C, nrow, padding)
                assert np.array_equal(got.cpu().numpy(), want), (n, C, nrow, padding)


def test_make_grid_defaults_and_a_list():
    x = _values(3, 3, 8, 8, 1)
    got = vis.make_grid([t.to(DEV) for t in x])
    assert np.array_equal(got.cpu().numpy(), V.make_grid(x.numpy()))


@pytest.mark.parametrize('H, W', [(5, 7), (8, 8)])
def test_make_grid_reads_slices_in_place(H, W):
    """Images that are slices of a wider buffer (image stride above C H W), and a base on a 4-byte but not a 16-byte boundary."""
    for n, C in ((3, 3), (11, 1)):
        wide = _values(n, 2 * C + 1, H, W, 7).to(DEV)
        for view in (wide[:, :C], wide[:, C + 1:]):
            assert view.stride(0) > C * H * W and not view.is_contiguous()
            assert np.array_equal(vis.make_grid(view, pad_value=0.5).cpu().numpy(), V.make_grid(view.cpu().numpy(), pad_value=0.5))
        flat = torch.rand(n * C * H * W + 1).to(DEV)
        odd = flat[1:].view(n, C, H, W)
        assert odd.data_ptr() % 16 == 4
        assert np.array_equal(vis.make_grid(odd, nrow=4).cpu().numpy(), V.make_grid(odd.cpu().numpy(), 4))


def test_vector_path_where_pixels_straddle_rows_or_sit_on_odd_words():
    """The 16-byte load path (H W % 4 == 0) where its 8-byte stores do not apply: a thread's four pixels run over the end of a
    row (W % 4 != 0), pairs start at an odd column or in an odd-sized plane (odd padding), and a grid starts at an odd atlas word."""
    for H, W, nrow, padding in ((4, 3, 8, 0), (4, 3, 8, 2), (2, 6, 8, 2), (2, 2, 8, 1), (1, 4, 2, 1)):
        for C in (1, 3):
            x = _values(3, C, H, W, 10 * H + W + C)
            atlas = vis._Atlas(DEV)
            pic = atlas.grid(vis.COPY, x.to(DEV), 'copy', nrow, padding, 0.5)
            assert atlas.rows[0][0][vis.D_VEC] == 1
            atlas.fetch()
            assert np.array_equal(atlas.host_view(pic).numpy(), V.make_grid(x.numpy(), nrow, padding, 0.5)), (H, W, nrow, padding, C)
    assert vis.grid_geometry(3, 1, 4, 2, 1)[3:] == (5, 11)                 # ... the odd-sized plane among them
    dot, x, m = _values(1, 3, 1, 1, 1), _values(3, 3, 8, 8, 2), -_values(11, 1, 8, 8, 3)
    atlas = vis._Atlas(DEV)
    pics = [atlas.grid(vis.COPY, dot.to(DEV), 'dot'), atlas.grid(vis.COPY, x.to(DEV), 'x'), atlas.grid(vis.EXP, m.to(DEV), 'm')]
    assert [atlas.pictures[p][0] % 2 for p in pics] == [0, 1, 1] and [r[0][vis.D_VEC] for r in atlas.rows] == [0, 1, 1]
    atlas.fetch()
    assert np.array_equal(atlas.host_view(pics[0]).numpy(), dot[0].numpy())
    assert np.array_equal(atlas.host_view(pics[1]).numpy(), V.make_grid(x.numpy()))
    assert _ulps(atlas.host_view(pics[2]).numpy(), V.make_grid(_exp32(m.numpy()))).max() <= 1


# ---- colours -------------------------------------------------------------------------------------------------------------------
def test_colour_seg_masks_matches_the_reference(monkeypatch):
    rs = np.random.RandomState(3)
    labels = torch.from_numpy(rs.randint(-1, 15, (4, 5, 7)).astype(np.int64))
    labels[0, 0, :3] = torch.tensor([-1, 0, 14])
    if R.reference_available():
        R.import_reference()
        import utils.misc as misc
        monkeypatch.chdir(R.REFERENCE_ROOT)
        want3, want4, palette = misc.colour_seg_masks(labels).numpy(), misc.colour_seg_masks(labels[:, None]).numpy(), '15'
    else:
        want3 = want4 = V.colour_seg_masks(labels.numpy())
        palette = V.PALETTE15
    for masks, want in ((labels, want3), (labels[:, None], want4), (labels.to(torch.int32), want3)):
        got = vis.colour_seg_masks(masks.to(DEV), palette)
        assert got.is_cuda and got.dtype == torch.int64 and tuple(got.shape) == (4, 3, 5, 7)
        assert np.array_equal(got.cpu().numpy(), want)
    vec = labels[:, :4, :4].contiguous()        # 16 pixels: four labels per thread
    assert np.array_equal(vis.colour_seg_masks(vec.to(DEV), V.load_palette()).cpu().numpy(), V.colour_seg_masks(vec.numpy()))


def test_a_label_beyond_the_palette_raises_in_visualise_outputs():
    g = S.load_case('nosample')
    batch = S.make_batch(g, DEV)
    batch['instances'][2, 0, 3, 3] = 15
    model, writer = S.StubModel(g, DEV), S.Writer()
    with pytest.raises(GenesisHipError, match='palette of 15 colours'):
        vis.visualise_outputs(model, batch, writer, 'val', 1, palette=V.PALETTE15)
    assert writer.calls == [] and model.training
    # ... and colour_seg_masks alone paints it black
    got = vis.colour_seg_masks(batch['instances'][2:3], V.PALETTE15)
    assert got[0, :, 3, 3].tolist() == [0, 0, 0]


def _argmax_case(K, B, H, W, seed):
    """K planes [B, 1, H, W] with exact ties, a NaN in plane 1 (plane 0 finite) and a NaN in plane 0."""
    rs = np.random.RandomState(seed)
    p = (rs.randint(0, 4, (K, B, 1, H, W)) / 4.0).astype(np.float32)      # quarters: ties are frequent
    p[0, 0, 0, 0, 0] = np.nan
    if K > 1:
        p[1, 0, 0, 0, 0] = np.nan                                         # behind the first NaN: plane 0 still wins
        p[1, -1, 0, -1, -1] = np.nan
        p[:, 0, 0, -1, 0] = 0.75                                          # all equal: the lowest k
    if K > 2:
        p[2, -1, 0, -1, -1] = np.nan                                      # a second NaN behind plane 1's
    return torch.from_numpy(p)


@pytest.mark.parametrize('K', [1, 2, 32])
@pytest.mark.parametrize('H, W', [(5, 7), (8, 8)])
def test_argmax_colour(K, H, W):
    B = 3
    stacked = _argmax_case(K, B, H, W, K)
    want_idx = torch.argmax(torch.cat(list(stacked.unbind(0)), 1), 1, True)
    assert int(want_idx[0, 0, 0, 0]) == 0 and int(want_idx[0, 0, -1, 0]) == 0 and (K == 1 or int(want_idx[-1, 0, -1, -1]) == 1)
    want = V.make_grid(V.colour_seg_masks(want_idx.numpy(), PALETTE32).astype(np.float32))
    dev = stacked.to(DEV)
    flat = torch.zeros(K * B * H * W + 1, device=DEV)
    flat[1:] = dev.reshape(-1)
    forms = {'packed': list(dev.unbind(0)), 'separate': [p.clone() for p in dev.unbind(0)],
             'packed, odd base': list(flat[1:].view(K, B, 1, H, W).unbind(0))}
    for name, planes in forms.items():
        atlas = vis._Atlas(DEV, vis.load_palette(PALETTE32))
        pic = atlas.argmax_grid(planes, name)
        assert bool(atlas.rows[0][0][vis.D_PACKED]) == (name != 'separate' or K == 1)      # one plane is its own packing
        assert atlas.fetch() == 0
        assert np.array_equal(atlas.host_view(pic).numpy(), want), name
    # an argmax beyond the palette is counted, and painted black
    if K == 32:
        atlas = vis._Atlas(DEV, vis.load_palette(PALETTE32[:4]))
        pic = atlas.argmax_grid(forms['packed'], 'short palette')
        assert atlas.fetch() == int((want_idx >= 4).sum())
        got = atlas.host_view(pic).numpy()
        inside = V.make_grid(np.broadcast_to((want_idx < 4).numpy(), (B, 3, H, W)).astype(np.float32)) > 0
        assert np.array_equal(got[inside], want[inside]) and not got[~inside].any()


def test_exp_kind():
    special = np.array([-1e10, -np.inf, 0.0, -1e-3, -87.5, 1.0], np.float32)
    for shape in ((1, 1, 2, 3), (3, 1, 8, 8), (3, 1, 5, 7)):                # the bare image; the vector path; the scalar path
        x = np.resize(special, shape).astype(np.float32)
        atlas = vis._Atlas(DEV)
        pic = atlas.grid(vis.EXP, torch.from_numpy(x).to(DEV), 'exp')
        atlas.fetch()
        got = atlas.host_view(pic).numpy()
        want = V.make_grid(_exp32(x))
        assert got.shape == want.shape
        exact = V.make_grid(np.isin(x, special[:3]).astype(np.float32)) > 0
        assert exact.any() and np.array_equal(got[exact], want[exact])
        assert set(np.unique(got[exact]).tolist()) == {0.0, 1.0}
        assert _ulps(got, want).max() <= 1


# ---- visualise_outputs ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('packed', [False, True])
@pytest.mark.parametrize('case', S.CASES)
def test_visualise_outputs_matches_the_reference(case, packed, capsys):
    g = S.load_case(case)
    model, writer = S.StubModel(g, DEV, packed=packed), S.Writer()
    batch = S.make_batch(g)                                                 # a host batch, as the reference's loader gives
    if 'instances' in batch and packed:
        batch = {k: v.to(DEV) for k, v in batch.items()}
    vis.visualise_outputs(model, batch, writer, 'val', int(g['iter_idx']), palette=V.PALETTE15)
    want = S.recorded_calls(g)
    assert [c[0] for c in writer.calls] == [t for t, _ in want]
    for (tag, got, step), (_, ref) in zip(writer.calls, want):
        assert torch.is_tensor(got) and not got.is_cuda and step == int(g['iter_idx']), tag
        got = got.numpy()
        assert got.shape == ref.shape and got.dtype == ref.dtype, tag
        if 'log_m' in tag:
            assert _ulps(got, ref).max() <= 1, tag
        else:
            assert np.array_equal(got, ref), tag
    assert model.training
    assert model.seen[0] == ('forward', False, (8, 3, 8, 8), 'cuda')
    assert model.seen[1] == ('sample', False, 8, model.K_steps)
    assert ('Sampling not implemented for this model.' in capsys.readouterr().out) == (case == 'nosample')


def test_visualise_outputs_restores_train_mode_when_the_forward_raises():
    g = S.load_case('monet')
    model, writer = S.StubModel(g, DEV, fail=True), S.Writer()
    with pytest.raises(RuntimeError, match='stub forward fails'):
        vis.visualise_outputs(model, S.make_batch(g), writer, 'val', 3, palette=V.PALETTE15)
    assert model.training and model.seen == [('forward', False, (8, 3, 8, 8), 'cuda')] and writer.calls == []


class _Recording(object):
    """A model that keeps what its forward pass and sample returned."""

    def __init__(self, model):
        self.model, self.K_steps = model, model.K_steps

    def eval(self):
        self.model.eval()
        return self

    def train(self, mode=True):
        self.model.train(mode)
        return self

    def parameters(self):
        return self.model.parameters()

    def __call__(self, x):
        self.forward_out = self.model(x)
        return self.forward_out

    def sample(self, batch_size, K_steps):
        self.sample_out = self.model.sample(batch_size, K_steps)
        return self.sample_out


def test_visualise_outputs_on_a_real_model():
    import genesis_amd.genesisv2_config as G
    from tests.common import Golden
    gold = Golden('tiny')
    cfg = AttrDict(dict(dict(dynamic_K=False), **dict(gold.cfg, debug=False, multi_gpu=False)))
    torch.manual_seed(0)
    net = G.load(cfg)
    net.load_state_dict(gold.weights(net.state_dict()))
    model, writer = _Recording(net.to(DEV).train()), S.Writer()
    rs = np.random.RandomState(5)
    S_ = gold.S
    batch = {'input': torch.from_numpy(rs.rand(10, 3, S_, S_).astype(np.float32)),
             'instances': torch.from_numpy(rs.randint(-1, 15, (10, 1, S_, S_)).astype(np.int64))}
    vis.visualise_outputs(model, batch, writer, 'train', 40, palette=V.PALETTE15)
    assert net.training
    recon, _, stats, _, _ = model.forward_out
    K = gold.K
    host = lambda t: t.detach().cpu().numpy()  # noqa: E731
    want = [('train_input', V.make_grid(batch['input'][:8].numpy())), ('train_recon', V.make_grid(host(recon))),
            ('train_instances_gt', V.make_grid(V.colour_seg_masks(batch['instances'][:8].numpy())))]
    for field, tag in (('log_m_k', 'train_instances'), ('log_m_r_k', 'train_instances_r')):
        idx = torch.argmax(torch.cat([m.detach().cpu() for m in stats[field]], 1), 1, True)
        want.append((tag, V.make_grid(V.colour_seg_masks(idx.numpy()))))
    for key in ('mx_r_k', 'x_r_k', 'log_m_k', 'log_m_r_k'):
        for step, val in enumerate(stats[key]):
            want.append(('train_%s/k%d' % (key, step), V.make_grid(_exp32(host(val)) if 'log' in key else host(val))))
    n_forward = len(want)
    assert n_forward == 5 + 4 * K
    calls = writer.calls
    assert [c[0] for c in calls[:n_forward]] == [t for t, _ in want]
    for (tag, got, _), (_, ref) in zip(calls, want):
        got = got.numpy()
        assert not torch.is_tensor(ref) and got.shape == ref.shape and got.dtype == ref.dtype, tag
        if 'log_m' in tag:
            assert _ulps(got, ref).max() <= 1, tag
        else:
            assert np.array_equal(got, ref), tag
    # the sample draws its own noise: tags and shapes only
    sample, sstats = model.sample_out
    shape = V.make_grid(np.zeros((8, 3, S_, S_), np.float32)).shape
    assert [c[0] for c in calls[n_forward:]] == ['samples'] + ['gen_%s/k%d' % (key, k) for key in ('x_k', 'log_m_k', 'mx_k')
                                                                  for k in range(K)]
    for tag, got, _ in calls[n_forward:]:
        assert tuple(got.shape) == shape and got.dtype == torch.float32 and not got.is_cuda, tag


# ---- sheets --------------------------------------------------------------------------------------------------------------------
class _SheetModel(object):
    """forward() and sample() hand out K = 2 slots of 8 x 8 in sixteenths (never 8 / 16: 127.5 is a rounding tie), masks of
    exp = 1, 0 and 0.25."""

    def __init__(self, B, packed, scope, seed=11):
        rs = np.random.RandomState(seed)
        sixteenths = np.array([k for k in range(17) if k != 8], np.float32) / 16.0
        pick = lambda *shape: torch.from_numpy(rs.choice(sixteenths, shape)).to(DEV)  # noqa: E731
        logs = np.array([0.0, -1e10, np.log(np.float32(0.25))], np.float32)
        logm = lambda *shape: torch.from_numpy(rs.choice(logs, shape)).to(DEV)  # noqa: E731
        self.K, self.B, self.packed = 2, B, packed
        self.x, self.recon = pick(B, 3, 8, 8), pick(B, 3, 8, 8)
        self.t = {'x_r_k': pick(2, B, 3, 8, 8), 'log_m_k': logm(2, B, 1, 8, 8), 'log_m_r_k': logm(2, B, 1, 8, 8)}
        if scope:
            self.t['log_s_k'] = logm(2, B, 1, 8, 8)
        self.t['mx_k'] = self.t['x_r_k'] * self.t['log_m_k'].exp()
        self.param = torch.nn.Parameter(torch.zeros(1, device=DEV))

    def parameters(self):
        return iter([self.param])

    def _stats(self, names):
        out = AttrDict()
        for new, old in names.items():
            if old in self.t:
                out[new] = list(self.t[old].unbind(0)) if self.packed else [p.clone() for p in self.t[old].unbind(0)]
        return out

    def __call__(self, x):
        assert x.is_cuda
        return self.recon, None, self._stats({k: k for k in ('x_r_k', 'log_m_k', 'log_m_r_k', 'log_s_k')}), None, None

    def sample(self, batch_size, K_steps):
        assert (batch_size, K_steps) == (self.B, self.K)
        return self.recon, self._stats({'x_k': 'x_r_k', 'log_m_k': 'log_m_k', 'mx_k': 'mx_k', 'log_s_k': 'log_s_k'})


def _no_rounding_ties(sheet):
    """No element of the fp32 sheet within 1e-6 of a half-integer once scaled to 0..255: the uint8 sheet must then be exact."""
    scaled = np.clip(sheet.astype(np.float64), 0, 1) * 255.0
    return not (np.abs(scaled - np.floor(scaled) - 0.5) < 1e-6).any()


def _want_sheet(m, mask_field, generation=False):
    h = {k: v.cpu().numpy() for k, v in m.t.items()}
    first, rows = [], []
    for b in range(m.B):
        x_k, lm = [h['x_r_k'][k, b] for k in range(2)], [h[mask_field][k, b] for k in range(2)]
        mx = [h['mx_k'][k, b] for k in range(2)] if generation else [x * _exp32(l) for x, l in zip(x_k, lm)]
        first += [m.recon[b].cpu().numpy()] + [None, None] if generation else [m.x[b].cpu().numpy(), m.recon[b].cpu().numpy(), None]
        rows += [mx, x_k, [_exp32(l) for l in lm]]
        if 'log_s_k' in h:
            first.append(None)
            rows.append([_exp32(h['log_s_k'][k, b]) for k in range(2)])
    return V.sheet_fp32(first, rows, 2)


@pytest.mark.parametrize('B, packed, scope', [(1, True, True), (2, False, False), (2, True, False)])
def test_reconstruction_sheet(B, packed, scope, tmp_path):
    m = _SheetModel(B, packed, scope)
    for field in (None, 'log_m_r_k'):
        fp32 = _want_sheet(m, field or 'log_m_k')
        assert _no_rounding_ties(fp32)
        got = vis.reconstruction_sheet(m, m.x.cpu(), mask_field=field)
        assert isinstance(got, np.ndarray) and got.dtype == np.uint8
        assert got.shape == (B * (4 if scope else 3) * 10 + 2, 3 * 10 + 2, 3)
        assert np.array_equal(got, V.to_u8_hwc(fp32))
    # ... and as a PNG, through the project's own decoder
    from genesis_amd.png import decode_png_batch
    path = str(tmp_path / 'sheet.png')
    vis.save_png(path, got)
    with open(path, 'rb') as f:
        _, u8 = decode_png_batch([f.read()], return_u8=True, device=DEV)
    assert np.array_equal(u8[0].cpu().numpy(), got)


def test_generation_sheet():
    m = _SheetModel(2, True, True)
    fp32 = _want_sheet(m, 'log_m_k', generation=True)
    assert _no_rounding_ties(fp32)
    got = vis.generation_sheet(m, 2, 2)
    assert got.shape == (2 * 4 * 10 + 2, 32, 3) and np.array_equal(got, V.to_u8_hwc(fp32))


def test_reconstruction_sheet_mask_field_rule_on_a_real_model():
    """GENESIS-V2 is recognised by the module of the model's class and shown with log_m_r_k; a model inside a wrapper is not
    recognised (documented) and gets log_m_k unless mask_field says otherwise."""
    import genesis_amd.genesisv2_config as G
    from tests.common import Golden
    gold = Golden('tiny')
    cfg = AttrDict(dict(dict(dynamic_K=False), **dict(gold.cfg, debug=False, multi_gpu=False)))
    torch.manual_seed(0)
    net = G.load(cfg)
    net.load_state_dict(gold.weights(net.state_dict()))
    net = net.to(DEV).eval()
    x = torch.from_numpy(np.random.RandomState(9).rand(1, 3, gold.S, gold.S).astype(np.float32))

    def sheet(model, field):
        torch.manual_seed(123)                                              # the same noise in every forward pass
        with torch.no_grad():
            return vis.reconstruction_sheet(model, x, mask_field=field)

    by_rule, r, k = sheet(net, None), sheet(net, 'log_m_r_k'), sheet(net, 'log_m_k')
    assert by_rule.shape == (4 * (gold.S + 2) + 2, (gold.K + 1) * (gold.S + 2) + 2, 3) and by_rule.dtype == np.uint8
    assert np.array_equal(r, sheet(net, 'log_m_r_k'))                      # repeatable, so the comparisons below mean something
    assert np.array_equal(by_rule, r) and not np.array_equal(r, k)
    assert np.array_equal(sheet(_Recording(net), None), k)
