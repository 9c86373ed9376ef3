"""The top-down attention captioner (--caption_model topdown): everything that needs no device.
Bounds: the kernel family's (tests/test_kernels_gpu.py rel_err): 1e-5 forward, 1e-4 gradients."""
import os

import numpy as np
import pytest
import torch

from topdown_util import CAP, TopDownRef, TorchOps, TorchLinearOp, nll, td_opt, cap_state, rel_err, grad_errs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, 'tests', 'golden', 'ref_topdown.npz')
FWD_TOL, GRAD_TOL = 1e-5, 1e-4
SMALL = dict(vocab_size=20, input_encoding_size=12, rnn_size=32, att_hid_size=16, fc_feat_size=64, att_feat_size=64)


def _store(opt, variant='cycle', dt=None):
    from lang2seg_amd._lib import F32
    from lang2seg_amd.nets.params import ParamStore
    return ParamStore(opt, 50, 81, 12, 1, 'cpu', F32 if dt is None else dt, variant)


def _gold():
    z = np.load(GOLD)
    opt = {k[4:]: int(z[k]) for k in z.files if k.startswith('opt.')}
    return z, opt


def test_restatement_reproduces_the_reference_fixture():
    """TopDownRef with the fixture's weights, in float32: the reference model's log-probabilities, criterion loss and the gradient of every
    parameter and of fc_feats / att_feats"""
    z, opt = _gold()
    mod = TopDownRef(opt)
    mod.load_state_dict({k[2:]: torch.from_numpy(z[k]) for k in z.files if k.startswith('w.')}, strict=True)
    fc = torch.from_numpy(z['fc_feats']).requires_grad_(True); att = torch.from_numpy(z['att_feats']).requires_grad_(True)
    seq, masks = torch.from_numpy(z['seq']), torch.from_numpy(z['masks'])
    lp = mod(fc, att, seq)
    assert tuple(lp.shape) == tuple(z['logprobs'].shape)
    loss = nll(lp, seq, masks)
    loss.backward()
    e = rel_err(lp, z['logprobs'])
    print('restatement vs reference: logprobs %.2e loss %.2e' % (e, abs(float(loss.detach()) - float(z['loss']))))
    assert e < FWD_TOL and abs(float(loss.detach()) - float(z['loss'])) < 1e-5 * max(1.0, abs(float(z['loss'])))
    errs = {k: rel_err(p.grad, z['g.' + k]) for k, p in mod.named_parameters()}
    errs['fc_feats'] = rel_err(fc.grad, z['g_fc_feats']); errs['att_feats'] = rel_err(att.grad, z['g_att_feats'])
    print('  grads worst %.2e (%s)' % (max(errs.values()), max(errs, key=errs.get)))
    assert set('g.' + k for k in errs if '_feats' not in k) == set(k for k in z.files if k.startswith('g.'))
    for k, v in errs.items():
        assert v < GRAD_TOL, (k, v)


@pytest.mark.parametrize('sizes', [dict(), SMALL])
def test_parameter_table_is_torchs(sizes):
    """keys, order and shapes under caption_model. are state_dict() of the restatement (default sizes, and a set with
    input_encoding_size != rnn_size != att_hid_size); every one is trainable; att2in2's core keys are gone"""
    opt = td_opt(**sizes)
    P = _store(opt)
    ref = {CAP + k: tuple(v.shape) for k, v in TopDownRef(opt).state_dict().items()}
    got = {k: tuple(v) for k, v in P.shapes.items() if k.startswith(CAP)}
    assert got == ref and list(got) == list(ref)
    assert all(k in P.offsets for k in ref)
    assert not any(k.startswith(CAP + 'core.' + n) for k in got for n in ('i2h', 'h2h', 'a2c'))
    R, IE = opt['rnn_size'], opt['input_encoding_size']
    assert got[CAP + 'core.att_lstm.weight_ih'] == (4 * R, IE + 2 * R) and got[CAP + 'core.lang_lstm.weight_ih'] == (4 * R, 2 * R)
    sd = P.state_dict()
    assert all(tuple(sd[k].shape) == ref[k] for k in ref)
    # the default captioner's table is what it was
    Pa = _store(dict(opt, caption_model='att2in2'))
    assert CAP + 'core.i2h.weight' in Pa.shapes and CAP + 'fc_embed.0.weight' not in Pa.shapes


def test_rejected_options_raise_value_errors_naming_them():
    from lang2seg_amd.nets.resnet_v1 import resnetv1
    from lang2seg_amd.nets.resnet_v1_cycle_response import resnetv1 as resnetv1_cr
    from lang2seg_amd.nets.vgg16 import vgg16
    for make in (resnetv1, resnetv1_cr):
        with pytest.raises(ValueError, match='caption_model') as e:
            make(td_opt(caption_model='adaatt'), batch_size=1, num_layers=101)
        assert 'att2in2' in str(e.value) and 'topdown' in str(e.value)
        with pytest.raises(ValueError, match='rnn_size'):
            make(td_opt(rnn_size=510), batch_size=1, num_layers=101)
        assert make(td_opt(), batch_size=1, num_layers=101).cap_model == 'topdown'
        assert make(td_opt(caption_model='att2in2'), batch_size=1, num_layers=101).cap_model == 'att2in2'
    # networks without a caption branch ignore the option, as before
    assert vgg16(td_opt(caption_model='adaatt', C4_feat_dim=512), batch_size=1).cap_model is None
    assert resnetv1(td_opt(caption_model='adaatt'), batch_size=1, num_layers=101, variant='spatial').cap_model is None


def test_state_dict_or_warm_start_of_the_other_captioner_names_the_flag(tmp_path, monkeypatch):
    from lang2seg_amd.utils import caption_ckpt as CK
    from lang2seg_amd.nets.params import ParamStore
    from oracle import weights as OW
    monkeypatch.setattr(ParamStore, 'refresh_shadow_full', lambda self: None)       # (the dtype shadow is rewritten by a device launch)
    opt = td_opt(**SMALL)
    P = _store(opt)
    a2 = {k: v for k, v in OW.make_state_dict(dict(opt, caption_model='att2in2'), seed=3).items() if k.startswith(CAP)}
    with pytest.raises(ValueError, match='--caption_model att2in2'):
        P.load_state_dict(a2)
    Pa = _store(dict(opt, caption_model='att2in2'))
    with pytest.raises(ValueError, match='--caption_model topdown'):
        Pa.load_state_dict(cap_state(opt))
    P.load_state_dict(cap_state(opt))                                          # its own: loads
    Pa.load_state_dict({'resnet.conv1.weight': np.zeros((64, 3, 7, 7), np.float32)})   # a detector's dict without a captioner: passes

    # --start_from: a model-best.pth of the other captioner
    class Net(object):
        def __init__(self, sd): self.sd = {k: torch.from_numpy(v) for k, v in sd.items()}
        def state_dict(self): return dict(self.sd)
        def load_state_dict(self, sd, strict=False): self.sd = dict(sd)
    d = tmp_path / 'refcoco_unc' / 'caption_log'
    d.mkdir(parents=True)
    (d / 'infos-best.pkl').write_bytes(b'')
    o = dict(opt, dataset_splitBy='refcoco_unc', start_from='caption_log')
    torch.save({k[len(CAP):]: torch.from_numpy(v) for k, v in a2.items()}, str(d / 'model-best.pth'))
    with pytest.raises(ValueError, match='--caption_model att2in2'):
        CK.load_caption_weights(Net(cap_state(opt)), o, str(tmp_path))
    torch.save({k[len(CAP):]: torch.from_numpy(v) for k, v in cap_state(opt).items()}, str(d / 'model-best.pth'))
    with pytest.raises(ValueError, match='--caption_model topdown'):
        CK.load_caption_weights(Net(a2), dict(o, caption_model='att2in2'), str(tmp_path))
    # and the reference-format file of THIS captioner loads strictly, key for key
    net = Net(cap_state(opt, seed=1))
    assert CK.load_caption_weights(net, o, str(tmp_path))
    want = cap_state(opt)
    assert set(net.sd) == set(want) and all(np.array_equal(np.asarray(net.sd[k]), want[k]) for k in want)


@pytest.mark.parametrize('variant', ['cycle', 'cycle_response'])
def test_new_keys_follow_the_solver_rule_and_travel_as_masters(variant):
    """the variant's param-group rule (bias keys: the bias group - no weight decay unless BIAS_DECAY, lr doubled with DOUBLE_BIAS; no
    language-side factor in the cycle solvers); the captioner's own tensors are read as fp32 masters, so never shadow-only; the gradient
    buckets of the data-parallel plan cover them"""
    from lang2seg_amd._lib import BF16
    from lang2seg_amd.nets.variants import solver_cfg
    from lang2seg_amd import parallel
    sc = solver_cfg(variant)
    P = _store(td_opt(**SMALL), variant, BF16)
    new = [k for k in P.trainable if k.startswith((CAP + 'core.att_lstm', CAP + 'core.lang_lstm', CAP + 'fc_embed'))]
    assert len(new) == 10
    for k in new:
        f, wd = P.param_group(k, sc.TRAIN.DOUBLE_BIAS, sc.TRAIN.BIAS_DECAY)
        assert f == (2.0 if ('bias' in k and sc.TRAIN.DOUBLE_BIAS) else 1.0), (k, f)
        assert wd == (0 if ('bias' in k and not sc.TRAIN.BIAS_DECAY) else 1), (k, wd)
        assert not P.shadow_only(k), k
    for lo, hi, so in P.shadow_only_runs():
        if so:
            assert not any(lo <= P.offsets[k] < hi for k in new)
    cap_hi = max(P.offsets[k] + int(np.prod(P.shapes[k])) for k in P.trainable if k.startswith(CAP))
    assert all(P.offsets[k] < cap_hi for k in new)
    assert P.defer_range[0] == P.offsets[CAP + 'att_embed.0.bias']              # att_embed still opens the heads stage's range


def test_tools_accept_the_option():
    """tools/opt.py hands --caption_model topdown on, and a network built from those options is the top-down one"""
    import sys
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import opt as tools_opt
    from lang2seg_amd.nets.params import caption_config, caption_shapes
    o = dict(tools_opt.parse_opt(['--caption_model', 'topdown']))
    assert o['caption_model'] == 'topdown' and caption_config(o) == 'topdown'
    assert dict(tools_opt.parse_opt([]))['caption_model'] == 'att2in2'
    o.setdefault('vocab_size', 60)
    assert CAP + 'core.att_lstm.weight_ih' in caption_shapes(o)


@pytest.mark.parametrize('S,masks', [(1, False), (4, False), (4, True)])
def test_captioner_host_order_with_torch_kernels(S, masks, monkeypatch):
    """nets/captioners.py TopDown (pre / fwd / bwd through Network._caption_*) with every entry point it calls restated in torch (topdown_util.TorchOps): the
    host's part - which buffer, column block, transposed block and key goes into which launch, in which order - gives the restatement's
    log-probabilities, loss, parameter gradients and d(att_feats) / d(fc_feats), with injected dropout masks and without"""
    from lang2seg_amd import ops as O
    from lang2seg_amd._lib import F32
    from lang2seg_amd.nets import resnet_v1 as RN
    from lang2seg_amd.nets.params import ParamStore
    for n in TorchOps.NAMES:
        monkeypatch.setattr(O, n, getattr(TorchOps, n), raising=False)
    monkeypatch.setattr(ParamStore, 'refresh_shadow_full', lambda self: None)
    opt = td_opt(**SMALL)
    R, IE, AH, V, L = opt['rnn_size'], opt['input_encoding_size'], opt['att_hid_size'], opt['vocab_size'], 196
    net = RN.resnetv1(opt, batch_size=1, num_layers=50)
    net.device, net.dt = 'cpu', F32
    net.P = P = ParamStore(opt, 50, 81, 12, 1, 'cpu', F32)
    sd = cap_state(opt, seed=4)
    P.load_state_dict(sd)
    net.wT = {CAP + 'core.' + k: (P.view(CAP + 'core.' + k).view(P.shapes[CAP + 'core.' + k]).t().contiguous().view(-1),) + tuple(P.shapes[CAP + 'core.' + k])
              for k in ('att_lstm.weight_ih', 'att_lstm.weight_hh', 'lang_lstm.weight_ih', 'lang_lstm.weight_hh', 'attention.h2att.weight')}
    net.att_embed = TorchLinearOp(P, CAP + 'att_embed.0.weight', CAP + 'att_embed.0.bias')
    g = torch.Generator().manual_seed(3 + S)
    fc, att = torch.randn(opt['fc_feat_size'], generator=g), torch.randn(L, opt['att_feat_size'], generator=g)
    seq = torch.zeros(1, S + 2, dtype=torch.int64); seq[0, 1:S + 1] = torch.randint(1, V + 1, (S,), generator=g)
    seq[0, S] = 0                                                               # S input tokens: the start token and S - 1 words
    cm = torch.ones(1, S + 2)
    mk = lambda *s: (torch.rand(*s, generator=g) > 0.5).float() / 0.5
    drops = dict(att=mk(L, R), fc=mk(R), xt=mk(S, IE), out=mk(S, R)) if masks else {}
    net.training, net.keep_logprobs, net._cap_loss_weight = True, True, 1.0
    net.parity = dict(drops=drops)
    net.t = {'fc_feats': fc.clone()}
    d = dict(S=S, cap_in=seq[0, :S].clone(), cap_tgt=seq[0, 1:S + 1].clone(), cap_mask=cm[0, 1:S + 1].clone())
    loss = torch.zeros(8)
    net._cap_pre = None
    net._caption_fwd(d, att.clone(), loss)
    P.grad.zero_()
    datt = net._caption_bwd(d, att.clone())
    for f in net._cap_deferred:
        f()
    mod = TopDownRef(opt)
    mod.load_state_dict({k[len(CAP):]: torch.from_numpy(v) for k, v in sd.items()})
    fcr, attr = fc.clone().view(1, -1).requires_grad_(True), att.clone().view(1, L, -1).requires_grad_(True)
    lp = mod(fcr, attr, seq, drops)
    assert lp.shape[1] == S
    ref = nll(lp, seq, cm)
    ref.backward()
    assert rel_err(net.t['cap.logp'], lp[0]) < FWD_TOL and abs(float(loss[5]) - float(ref.detach())) < 1e-5
    assert rel_err(datt, attr.grad) < GRAD_TOL and rel_err(net.t['cap.dfc'], fcr.grad) < GRAD_TOL
    ref_g = {k: p.grad for k, p in mod.named_parameters()}
    for k, e in grad_errs({k: P.view(CAP + k, P.grad) for k in ref_g}, ref_g).items():
        assert e < GRAD_TOL, (k, e)
