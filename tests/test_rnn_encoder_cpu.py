"""The general expression encoder (rnn_type lstm / gru / rnn, stacked layers, one or two directions): everything that needs no device."""
import os
import sys

import numpy as np
import pytest
import torch

from rnn_encoder_util import CONFIGS, PRE, enc_opt, torch_rnn, rnn_state, make_sd, LayeredRNN, TorchOps, run_module, rel_err, torch_encoder

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _store(opt, variant='cycle', dt=None):
    from lang2seg_amd._lib import F32
    from lang2seg_amd.nets.params import ParamStore
    if variant == 'vgg':
        opt = dict(opt, C4_feat_dim=512)
    return ParamStore(opt, 50, 81, 12, 0 if variant == 'vgg' else 1, 'cpu', F32 if dt is None else dt, variant)


@pytest.mark.parametrize('typ,layers,bidir', CONFIGS)
def test_parameter_table_is_torchs(typ, layers, bidir):
    """keys, order and shapes under rnn_encoder.rnn. are torch.nn.<cell>(word_vec_size, hidden, layers, bidirectional).state_dict()'s;
    the dynamic-filter FCs read layers x directions x hidden inputs"""
    opt = enc_opt(typ, layers, bidir, H=64)
    P = _store(opt)
    ref = {PRE + k: tuple(v.shape) for k, v in torch_rnn(typ, opt['word_vec_size'], 64, layers, bidir).state_dict().items()}
    got = {k: tuple(v) for k, v in P.shapes.items() if k.startswith(PRE)}
    assert got == ref and list(got) == list(ref)
    assert all(k in P.offsets for k in ref)                                   # every one trainable, in the flat buffer
    assert tuple(P.shapes['dynamic_fc_0.weight']) == (1024, layers * (2 if bidir else 1) * 64)
    sd = P.state_dict()
    assert all(tuple(sd[k].shape) == ref[k] for k in ref)


@pytest.mark.parametrize('variant', ['baseline', 'spatial', 'response', 'vgg', 'cycle', 'cycle_response'])
def test_encoder_keys_in_the_language_group_and_never_shadow_only(variant):
    from lang2seg_amd._lib import BF16
    from lang2seg_amd.nets.variants import SOLVERS, solver_cfg
    sc = solver_cfg(variant)
    mult = SOLVERS[variant]['lang_lr_mult']
    for typ, layers, bidir in CONFIGS:
        P = _store(enc_opt(typ, layers, bidir, H=64), variant, BF16)
        keys = [k for k in P.trainable if k.startswith('rnn_encoder.')]
        assert len(keys) == 3 + 4 * layers * (2 if bidir else 1)
        for k in keys:
            f, wd = P.param_group(k, sc.TRAIN.DOUBLE_BIAS, sc.TRAIN.BIAS_DECAY)
            assert f == mult * (2.0 if ('bias' in k and sc.TRAIN.DOUBLE_BIAS) else 1.0), (variant, k, f)
            assert wd == (0 if ('bias' in k and not sc.TRAIN.BIAS_DECAY) else 1)
            assert not P.shadow_only(k), k                                    # fp32 masters read by the kernels
        for lo, hi, so in P.shadow_only_runs():
            if so:
                assert not any(lo <= P.offsets[k] < hi for k in keys)


def test_rejected_options_raise_value_errors_naming_them():
    from lang2seg_amd.nets.resnet_v1 import resnetv1
    from lang2seg_amd.nets.vgg16 import vgg16
    for bad, name in ((dict(rnn_type='foo'), 'rnn_type'), (dict(variable_lengths=0), 'variable_lengths'), (dict(rnn_num_layers=0), 'rnn_num_layers'),
                      (dict(rnn_hidden_size=6), 'rnn_hidden_size')):
        opt = enc_opt('lstm', 1, 1); opt.update(bad)
        for make in (lambda: resnetv1(opt, batch_size=1, num_layers=101), lambda: vgg16(dict(opt, C4_feat_dim=512), batch_size=1)):
            with pytest.raises(ValueError, match=name):
                make()
    for typ, layers, bidir in CONFIGS:                                        # and the seven configurations construct
        assert resnetv1(enc_opt(typ, layers, bidir), batch_size=1, num_layers=101).enc[:3] == (typ, layers, 2 if bidir else 1)


def test_state_dict_of_another_encoder_is_an_error_naming_the_flag():
    P = _store(enc_opt('lstm', 1, 1, H=64))
    gru = rnn_state(torch_rnn('gru', 512, 64, 2, 1))
    with pytest.raises(ValueError, match='rnn_type') as e:
        P.load_state_dict(gru)
    assert 'rnn_num_layers' in str(e.value) and 'bidirectional' not in str(e.value)
    with pytest.raises(ValueError, match='bidirectional'):
        P.check_encoder_keys(rnn_state(torch_rnn('lstm', 512, 64, 1, 0)))
    with pytest.raises(ValueError, match='rnn_num_layers'):
        _store(enc_opt('gru', 2, 1, H=64)).check_encoder_keys(rnn_state(torch_rnn('gru', 512, 64, 1, 1)))
    P.check_encoder_keys(rnn_state(torch_rnn('lstm', 512, 64, 1, 1)))         # its own: passes
    P.check_encoder_keys({'resnet.conv1.weight': np.zeros((64, 3, 7, 7), np.float32)})   # a detector's dict without an encoder: passes


@pytest.mark.parametrize('typ,layers,bidir', CONFIGS)
def test_layered_oracle_is_the_module(typ, layers, bidir):
    """the util's layer-by-layer form (needed to put a given mask between layers) equals the one module call, values and gradients"""
    mod = torch_rnn(typ, 24, 16, layers, bidir, seed=5)
    x = torch.randn(5, 24, generator=torch.Generator().manual_seed(1))
    w = torch.randn(layers * (2 if bidir else 1) * 16, generator=torch.Generator().manual_seed(2))
    h_ref = run_module(mod, x)
    (h_ref * w).sum().backward()
    lay = LayeredRNN(typ, mod.state_dict(), layers, bidir)
    h = lay.forward(x)
    (h * w).sum().backward()
    assert rel_err(h, h_ref) < 1e-6
    for k, p in mod.named_parameters():
        assert rel_err(lay.p[k].grad, p.grad) < 1e-5, k


@pytest.mark.parametrize('typ,layers,bidir', CONFIGS)
def test_encoder_host_order_with_torch_kernels(typ, layers, bidir, monkeypatch):
    """Network._encoder_fwd / _encoder_bwd with every entry point they call restated in torch (rnn_encoder_util.TorchOps): the host's
    part - which buffer, slice, key and mask goes into which launch, in which order, for every layer and direction - gives torch's
    hidden and torch's gradients.  (The kernels behind the entry points: tests/test_rnn_encoder_gpu.py.)"""
    from lang2seg_amd import ops as O
    from lang2seg_amd._lib import F32
    from lang2seg_amd.nets import resnet_v1 as R
    from lang2seg_amd.nets.params import ParamStore
    for n in TorchOps.NAMES:
        monkeypatch.setattr(O, n, getattr(TorchOps, n))
    monkeypatch.setattr(R.resnetv1, '_ENC_STEP', {c: (getattr(TorchOps, c + '_step_fwd'), getattr(TorchOps, c + '_step_bwd')) for c in ('lstm', 'gru', 'rnn')})
    monkeypatch.setattr(ParamStore, 'refresh_shadow_full', lambda self: None)
    H, ndir = 64, 2 if bidir else 1
    opt = enc_opt(typ, layers, bidir, H=H)
    net = R.resnetv1(opt, batch_size=1, num_layers=50)
    net.device, net.dt = 'cpu', F32
    net.P = P = ParamStore(opt, 50, 81, 12, 1, 'cpu', F32)
    sd = {k: v for k, v in make_sd(opt, seed=3).items() if k.startswith('rnn_encoder.')}
    P.load_state_dict(sd)
    net.wT = {k: (P.view(k).view(P.shapes[k]).t().contiguous().view(-1),) + tuple(P.shapes[k]) for k in net._encoder_hh_keys()}
    g = torch.Generator().manual_seed(31)
    for T in (1, 4):
        for with_mask in ([False, True] if layers > 1 else [False]):
            labels = torch.randint(1, 60, (T,), generator=g)
            dhid = torch.randn(layers * ndir * H, generator=g)
            masks = [(torch.rand(T, ndir * H, generator=g) > 0.2).float() / 0.8 for _ in range(layers - 1)] if with_mask else None
            net.training, net.t = True, {}
            net.parity = dict(drops={'rnn_l%d' % l: masks[l] for l in range(layers - 1)} if with_mask else {})
            d = dict(T=T, labels=labels)
            hidden = net._encoder_fwd(d)
            P.grad.zero_()
            net._encoder_bwd(d, dhid)
            h32, g32 = torch_encoder(sd, opt, labels, masks, dhid, torch.float32)
            assert rel_err(hidden, h32) < 1e-5
            for k in g32:
                assert rel_err(P.view(k, P.grad).view(P.shapes[k]), g32[k]) < 1e-4, (T, with_mask, k)
            if with_mask:                                       # eval mode: the masks are not applied
                net.training = False
                h_eval = net._encoder_fwd(d).clone()
                assert rel_err(h_eval, torch_encoder(sd, opt, labels, None, dhid, torch.float32)[0]) < 1e-5


def test_eval_and_predict_tools_take_the_encoder_flags():
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import eval_common
    import predict
    for mod in (eval_common, predict):
        a = mod.parse_args(['--rnn_type', 'gru', '--rnn_num_layers', '2', '--bidirectional', '0'])
        assert (a['rnn_type'], a['rnn_num_layers'], a['bidirectional']) == ('gru', 2, 0)
        d = mod.parse_args([])                                                # not given: tools/opt.py's defaults apply
        assert (d['rnn_type'], d['rnn_num_layers'], d['bidirectional']) == (None, None, None)
    from opt import parse_opt
    o = parse_opt([])
    assert (o['rnn_type'], o['rnn_num_layers'], o['bidirectional']) == ('lstm', 1, 1)
