"""The adaptive-attention captioners (--caption_model adaatt | adaattmo): everything that needs no device.
Bounds: the kernel family's (tests/test_kernels_gpu.py rel_err): 1e-5 forward, 1e-4 gradients."""
import os

import numpy as np
import pytest
import torch

from adaatt_util import CAP, GATES, AdaAttRef, TorchOps, nll, ada_opt, cap_state, make_masks, rel_err, grad_errs
from topdown_util import TorchLinearOp, td_opt, cap_state as td_state

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FWD_TOL, GRAD_TOL = 1e-5, 1e-4
SMALL = dict(vocab_size=20, input_encoding_size=32, rnn_size=32, att_hid_size=32, fc_feat_size=64, att_feat_size=64)
MODELS = ['adaatt', 'adaattmo']
OTHER = {'adaatt': 'adaattmo', 'adaattmo': 'adaatt'}


def _store(opt, variant='cycle', dt=None):
    from lang2seg_amd._lib import F32
    from lang2seg_amd.nets.params import ParamStore
    return ParamStore(opt, 50, 81, 12, 1, 'cpu', F32 if dt is None else dt, variant)


def _gold(model):
    z = np.load(os.path.join(ROOT, 'tests', 'golden', 'ref_%s.npz' % model))
    opt = {k[4:]: int(z[k]) for k in z.files if k.startswith('opt.')}
    return z, dict(opt, caption_model=model)


@pytest.mark.parametrize('model', MODELS)
def test_restatement_reproduces_the_reference_fixture(model):
    """AdaAttRef with the fixture's weights, in float32: the reference model's log-probabilities, criterion loss and the gradient of every
    parameter and of fc_feats / att_feats"""
    z, opt = _gold(model)
    mod = AdaAttRef(opt)
    mod.load_state_dict({k[2:]: torch.from_numpy(z[k]) for k in z.files if k.startswith('w.')}, strict=True)
    fc = torch.from_numpy(z['fc_feats']).requires_grad_(True); att = torch.from_numpy(z['att_feats']).requires_grad_(True)
    seq, masks = torch.from_numpy(z['seq']), torch.from_numpy(z['masks'])
    lp = mod(fc, att, seq)
    assert tuple(lp.shape) == tuple(z['logprobs'].shape) and lp.shape[1] == 6
    loss = nll(lp, seq, masks)
    loss.backward()
    e = rel_err(lp, z['logprobs'])
    print('%s restatement vs reference: logprobs %.2e loss %.2e' % (model, e, abs(float(loss.detach()) - float(z['loss']))))
    assert e < FWD_TOL and abs(float(loss.detach()) - float(z['loss'])) < 1e-5 * max(1.0, abs(float(z['loss'])))
    ref_g = {k: z['g.' + k] for k, _ in mod.named_parameters()}
    errs = grad_errs({k: p.grad for k, p in mod.named_parameters()}, ref_g)
    errs['fc_feats'] = rel_err(fc.grad, z['g_fc_feats']); errs['att_feats'] = rel_err(att.grad, z['g_att_feats'])
    print('  grads worst %.2e (%s)' % (max(errs.values()), max(errs, key=errs.get)))
    assert len(ref_g) == 33 and set('g.' + k for k in ref_g) == set(k for k in z.files if k.startswith('g.'))
    for k, v in errs.items():
        assert v < GRAD_TOL, (k, v)


@pytest.mark.parametrize('sizes', [dict(), SMALL])
@pytest.mark.parametrize('model', MODELS)
def test_parameter_table_is_torchs(model, sizes):
    """keys, order and shapes under caption_model. are state_dict() of the restatement (default sizes and 32); 33 tensors, all trainable"""
    opt = ada_opt(model, **sizes)
    P = _store(opt)
    ref = {CAP + k: tuple(v.shape) for k, v in AdaAttRef(opt).state_dict().items()}
    got = {k: tuple(v) for k, v in P.shapes.items() if k.startswith(CAP)}
    assert got == ref and list(got) == list(ref) and len(got) == 33
    assert all(k in P.offsets for k in ref)
    R, G = opt['rnn_size'], GATES[model]
    for k in ('w2h', 'v2h', 'h2h.0'):
        assert got[CAP + 'core.lstm.%s.weight' % k][0] == G * R and got[CAP + 'core.lstm.%s.bias' % k] == (G * R,)
    sd = P.state_dict()
    assert all(tuple(sd[k].shape) == ref[k] for k in ref)
    # the other captioners' tables are what they were
    assert CAP + 'core.i2h.weight' in _store(dict(opt, caption_model='att2in2')).shapes
    assert CAP + 'core.att_lstm.weight_ih' in _store(dict(opt, caption_model='topdown')).shapes


@pytest.mark.parametrize('model', MODELS)
def test_rejected_options_raise_value_errors_naming_them(model):
    from lang2seg_amd.nets.resnet_v1 import resnetv1
    from lang2seg_amd.nets.resnet_v1_cycle_response import resnetv1 as resnetv1_cr
    from lang2seg_amd.nets.vgg16 import vgg16
    for make in (resnetv1, resnetv1_cr):
        with pytest.raises(ValueError, match='caption_model') as e:
            make(ada_opt('show_attend_tell'), batch_size=1, num_layers=101)
        assert all(n in str(e.value) for n in ('att2in2', 'topdown', 'adaatt', 'adaattmo'))
        with pytest.raises(ValueError, match='caption_model') as e:             # the pair is opt-in: the bare name is the error it always was
            make(ada_opt(model, adaatt=0), batch_size=1, num_layers=101)
        assert '--adaatt 1' in str(e.value) and 'att2in2' in str(e.value) and 'topdown' in str(e.value)
        for bad in (dict(att_hid_size=16), dict(input_encoding_size=256), dict(rnn_size=256)):
            with pytest.raises(ValueError, match='input_encoding_size') as e:
                make(ada_opt(model, **bad), batch_size=1, num_layers=101)
            assert 'rnn_size' in str(e.value) and 'att_hid_size' in str(e.value)
        with pytest.raises(ValueError, match='rnn_size'):
            make(ada_opt(model, rnn_size=30, input_encoding_size=30, att_hid_size=30), batch_size=1, num_layers=101)
        with pytest.raises(ValueError, match='num_layers') as e:
            make(ada_opt(model, num_layers=2), batch_size=1, num_layers=101)
        assert 'i2h' in str(e.value) and 'not built' in str(e.value)
        assert make(ada_opt(model), batch_size=1, num_layers=101).cap_model == model
    # networks without a caption branch ignore the option, as before
    assert vgg16(ada_opt(model, num_layers=2, C4_feat_dim=512), batch_size=1).cap_model is None
    assert resnetv1(ada_opt(model, att_hid_size=16), batch_size=1, num_layers=101, variant='spatial').cap_model is None


@pytest.mark.parametrize('model', MODELS)
def test_state_dict_or_warm_start_of_another_captioner_names_the_flag(model, tmp_path, monkeypatch):
    """att2in2 <-> adaatt, topdown <-> adaatt and adaatt <-> adaattmo (the pair shares every key: told apart by the rows of h2h.0)"""
    from lang2seg_amd.utils import caption_ckpt as CK
    from lang2seg_amd.nets.params import ParamStore
    from oracle import weights as OW
    monkeypatch.setattr(ParamStore, 'refresh_shadow_full', lambda self: None)
    opt = ada_opt(model, **SMALL)
    other = OTHER[model]
    mine, theirs = cap_state(opt), cap_state(dict(opt, caption_model=other))
    assert set(mine) == set(theirs)
    a2 = {k: v for k, v in OW.make_state_dict(dict(opt, caption_model='att2in2'), seed=3).items() if k.startswith(CAP)}
    td = td_state(td_opt(**SMALL))
    P = _store(opt)
    for sd, name in ((a2, 'att2in2'), (td, 'topdown'), (theirs, other)):
        with pytest.raises(ValueError, match=r'--caption_model %s \(this network: %s\)' % (name, model)):
            P.load_state_dict(sd)
    for o in ('att2in2', 'topdown', other):
        with pytest.raises(ValueError, match=r'--caption_model %s \(this network: %s\)' % (model, o)):
            _store(dict(opt, caption_model=o)).load_state_dict(mine)
    P.load_state_dict(mine)                                                    # its own: loads
    P.load_state_dict({'resnet.conv1.weight': np.zeros((64, 3, 7, 7), np.float32)})    # a detector's dict without a captioner: passes

    class Net(object):
        def __init__(self, sd): self.sd = {k: torch.from_numpy(v) for k, v in sd.items()}
        def state_dict(self): return dict(self.sd)
        def load_state_dict(self, sd, strict=False): self.sd = dict(sd)
    d = tmp_path / 'refcoco_unc' / 'caption_log'
    d.mkdir(parents=True)
    (d / 'infos-best.pkl').write_bytes(b'')
    o = dict(opt, dataset_splitBy='refcoco_unc', start_from='caption_log')
    strip = lambda sd: {k[len(CAP):]: torch.from_numpy(v) for k, v in sd.items()}
    for sd, name in ((a2, 'att2in2'), (td, 'topdown'), (theirs, other)):
        torch.save(strip(sd), str(d / 'model-best.pth'))
        with pytest.raises(ValueError, match=r'--caption_model %s \(this network: %s\)' % (name, model)):
            CK.load_caption_weights(Net(mine), o, str(tmp_path))
    torch.save(strip(mine), str(d / 'model-best.pth'))
    with pytest.raises(ValueError, match=r'--caption_model %s \(this network: att2in2\)' % model):
        CK.load_caption_weights(Net(a2), dict(o, caption_model='att2in2'), str(tmp_path))
    # and the reference-format file of THIS captioner loads strictly, key for key
    net = Net(cap_state(opt, seed=1))
    assert CK.load_caption_weights(net, o, str(tmp_path))
    assert set(net.sd) == set(mine) and all(np.array_equal(np.asarray(net.sd[k]), mine[k]) for k in mine)


def test_infos_check_accepts_the_names(tmp_path):
    """tools/train_common's infos-best.pkl check (caption_ckpt.check_infos): the saved caption_model must be the command line's"""
    import pickle
    from lang2seg_amd.utils import caption_ckpt as CK
    d = tmp_path / 'refcoco_unc' / 'caption_log'
    d.mkdir(parents=True)
    saved = dict(caption_model='adaattmo', rnn_type='lstm', rnn_size=512, num_layers=1)
    (d / 'infos-best.pkl').write_bytes(pickle.dumps({'opt': saved}, protocol=0))
    o = dict(ada_opt('adaattmo'), dataset_splitBy='refcoco_unc', start_from='caption_log')
    assert CK.check_infos(o, str(tmp_path))['opt']['caption_model'] == 'adaattmo'
    with pytest.raises(ValueError, match='caption_model'):
        CK.check_infos(dict(o, caption_model='adaatt'), str(tmp_path))


@pytest.mark.parametrize('variant', ['cycle', 'cycle_response'])
def test_new_keys_follow_the_solver_rule_and_travel_as_masters(variant):
    """the variant's param-group rule for the 24 core keys + fc_embed; read as fp32 masters, so never shadow-only (only att_embed.0.weight is);
    the flat layout keeps them in the captioner's range in front of att_embed"""
    from lang2seg_amd._lib import BF16
    from lang2seg_amd.nets.variants import solver_cfg
    sc = solver_cfg(variant)
    P = _store(ada_opt('adaattmo', **SMALL), variant, BF16)
    new = [k for k in P.trainable if k.startswith((CAP + 'core.', CAP + 'fc_embed'))]
    assert len(new) == 26
    for k in new:
        f, wd = P.param_group(k, sc.TRAIN.DOUBLE_BIAS, sc.TRAIN.BIAS_DECAY)
        assert f == (2.0 if ('bias' in k and sc.TRAIN.DOUBLE_BIAS) else 1.0), (k, f)
        assert wd == (0 if ('bias' in k and not sc.TRAIN.BIAS_DECAY) else 1), (k, wd)
        assert not P.shadow_only(k), k
    assert [k for k in P.trainable if k.startswith(CAP) and P.shadow_only(k)] == [CAP + 'att_embed.0.weight']
    for lo, hi, so in P.shadow_only_runs():
        if so:
            assert not any(lo <= P.offsets[k] < hi for k in new)
    cap_hi = max(P.offsets[k] + int(np.prod(P.shapes[k])) for k in P.trainable if k.startswith(CAP))
    assert all(P.offsets[k] < cap_hi for k in new)
    assert P.defer_range[0] == P.offsets[CAP + 'att_embed.0.bias']


def test_dropout_streams_differ():
    """_drop derives a mask's RNG stream from the sum of its name's character codes: the five new names, the four reused ones and the
    encoder's must not collide"""
    names = ['att', 'fc', 'xt', 'out', 'toph', 'fake', 'frl', 'hol', 'hA', 'word'] + ['rnn_l%d' % l for l in range(4)]
    sums = [sum(map(ord, n)) for n in names]
    assert len(set(sums)) == len(sums), dict(zip(names, sums))


@pytest.mark.parametrize('model', MODELS)
def test_tools_accept_the_option(model):
    import sys
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import opt as tools_opt
    from lang2seg_amd.nets.params import caption_config, caption_shapes
    o = dict(tools_opt.parse_opt(['--caption_model', model, '--adaatt', '1']))
    assert o['caption_model'] == model and caption_config(o) == model
    with pytest.raises(ValueError, match='--adaatt 1'):
        caption_config(dict(tools_opt.parse_opt(['--caption_model', model])))
    o.setdefault('vocab_size', 60)
    assert caption_shapes(o)[CAP + 'core.lstm.w2h.weight'] == (GATES[model] * o['rnn_size'], o['input_encoding_size'])
    for sh in ('train_cycle.sh', 'train_cycle_response.sh'):
        txt = open(os.path.join(ROOT, 'experiments', 'scripts', sh)).read()
        assert '--caption_model ${CAPTION_MODEL}' in txt and 'adaatt|adaattmo) ARGS="${ARGS} --adaatt 1"' in txt
    src = open(os.path.join(ROOT, 'tools', 'caption_model_bench.py')).read()
    assert repr(model) in src


@pytest.mark.parametrize('S,masks', [(1, False), (3, False), (3, True)])
@pytest.mark.parametrize('model', MODELS)
def test_captioner_host_order_with_torch_kernels(model, S, masks, monkeypatch):
    """nets/captioners.py AdaAtt (pre / fwd / bwd through Network._caption_*) with every entry point it calls restated in torch (adaatt_util.TorchOps): the host's
    part - which buffer, column block, transposed copy and key goes into which launch, in which order - gives the restatement's
    log-probabilities, loss, parameter gradients and d(att_feats) / d(fc_feats), with the nine injected dropout masks and without"""
    from lang2seg_amd import ops as O
    from lang2seg_amd._lib import F32
    from lang2seg_amd.nets import resnet_v1 as RN
    from lang2seg_amd.nets.params import ParamStore
    for n in TorchOps.NAMES:
        monkeypatch.setattr(O, n, getattr(TorchOps, n), raising=False)
    monkeypatch.setattr(ParamStore, 'refresh_shadow_full', lambda self: None)
    opt = ada_opt(model, **SMALL)
    R, IE, V, L = opt['rnn_size'], opt['input_encoding_size'], opt['vocab_size'], 196
    net = RN.resnetv1(opt, batch_size=1, num_layers=50)
    net.device, net.dt = 'cpu', F32
    net.P = P = ParamStore(opt, 50, 81, 12, 1, 'cpu', F32)
    sd = cap_state(opt, seed=4)
    P.load_state_dict(sd)
    net.wT = {CAP + 'core.' + k: (P.view(CAP + 'core.' + k).view(P.shapes[CAP + 'core.' + k]).t().contiguous().view(-1),) + tuple(P.shapes[CAP + 'core.' + k])
              for k in ('lstm.h2h.0.weight', 'lstm.r_h2h.weight')}
    net.att_embed = TorchLinearOp(P, CAP + 'att_embed.0.weight', CAP + 'att_embed.0.bias')
    g = torch.Generator().manual_seed(3 + S)
    fc, att = torch.randn(opt['fc_feat_size'], generator=g), torch.randn(L, opt['att_feat_size'], generator=g)
    seq = torch.zeros(1, S + 2, dtype=torch.int64); seq[0, 1:S + 1] = torch.randint(1, V + 1, (S,), generator=g)
    seq[0, S] = 0                                                               # S input tokens: the start token and S - 1 words
    cm = torch.ones(1, S + 2)
    drops = make_masks(opt, S, L, seed=7) if masks else {}
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
    mod = AdaAttRef(opt)
    mod.load_state_dict({k[len(CAP):]: torch.from_numpy(v) for k, v in sd.items()})
    fcr, attr = fc.clone().view(1, -1).requires_grad_(True), att.clone().view(1, L, -1).requires_grad_(True)
    lp = mod(fcr, attr, seq, drops)
    assert lp.shape[1] == S
    ref = nll(lp, seq, cm)
    ref.backward()
    assert rel_err(net.t['cap.logp'], lp[0]) < FWD_TOL and abs(float(loss[5]) - float(ref.detach())) < 1e-5
    assert rel_err(datt, attr.grad) < GRAD_TOL and rel_err(net.t['cap.dfc'], fcr.grad) < GRAD_TOL
    ref_g = {k: p.grad for k, p in mod.named_parameters()}
    assert len(ref_g) == 33
    for k, e in grad_errs({k: P.view(CAP + k, P.grad) for k in ref_g}, ref_g).items():
        assert e < GRAD_TOL, (k, e)
