"""The top-down attention captioner on the device (csrc/caption_step.hip and nets/captioners.py TopDown)
against the torch restatement of tests/topdown_util.py, which tests/test_topdown_cpu.py pins to the reference's own model.
Bounds: the kernel family's (tests/test_kernels_gpu.py rel_err) 1e-5 forward and 1e-4 gradients; 1e-4 on losses in exact-f32 mode; bf16:
losses within 1e-2 and cosine >= 0.99 per gradient tensor against the f32 device step.

Worst values measured on an MI355X (this file's own prints):
  step entries                 h / c 5.9e-07, gradients 1.6e-06 (five shapes)
  network vs oracle, f32       losses 1.8e-07, fc / att features 1.4e-06, d(att_feats) 7.5e-07, d(fc_feats) 2.9e-07; captioner gradients
                               2.2e-06 (cycle), 1.4e-06 (cycle, masks), 2.6e-05 (cycle_response), 1.3e-06 (cycle_response, masks)
  network bf16 vs f32          losses 1.5e-03, lowest cosine 0.9985 (d(att_feats))
  reference fixture            log-probabilities 1.5e-07, loss 0, gradients 1.6e-06

The cycle_response step without masks is the hard one: its features are nearly uniform, and the gradients of what enters the attention's tanh
alike for every location (h2att.*, ctx2att.bias) are sums over the locations that cancel to 1e-7 of their terms (the softmax ignores a common
shift).  With the plain form of that sum the device was 2.8e-04 off a float64 evaluation there, and a float32 autograd pass 3.0e-04; the device
now takes the sum centred on its weighted mean (l2s_cap_att_bwd_step_centered: 5e-06), and the oracle evaluates its captioner in float64
(topdown_util.TopDownOracleNet.caption)."""
import hashlib
import os

import numpy as np
import pytest
import torch

from rnn_encoder_util import edge_step_inputs
from topdown_util import (CAP, STEP_SHAPES, TopDownRef, TopDownOracleNet, core_reference, rel_err, grad_errs, cosine, nll, td_opt, make_sd, cap_state)

pytestmark = pytest.mark.gpu

DEV = 'cuda'
FWD_TOL, GRAD_TOL, LOSS_TOL = 1e-5, 1e-4, 1e-4
BF16_LOSS_RTOL, BF16_COS = 1e-2, 0.99
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, 'tests', 'golden', 'ref_topdown.npz')


def ops():
    from lang2seg_amd import ops as O
    return O


# ------------------------------------------------------------------ 1. the step entries alone
def _run_core(O, ref, R, IE, AH, S, L):
    """the core through the two step entries + the attention / linear entries around them, in the network's decomposition; returns the
    per-step states and the gradients under the restatement's names"""
    G, Ka = 4 * R, IE + 2 * R
    sd = {k: v.detach().to(DEV).contiguous() for k, v in ref['core'].state_dict().items()}
    flat = lambda k: sd[k].view(-1)
    T = lambda k: sd[k].t().contiguous().view(-1)
    z = lambda *s: torch.zeros(*s, device=DEV)
    xt, fc, att, patt, dout = (ref[k].to(DEV).contiguous() for k in ('xt', 'fc', 'att', 'p_att', 'dout'))
    wa_ih, wa_hh, wl_ih, wl_hh = flat('att_lstm.weight_ih'), flat('att_lstm.weight_hh'), flat('lang_lstm.weight_ih'), flat('lang_lstm.weight_hh')
    h2w, h2b, aw, ab = flat('attention.h2att.weight'), sd['attention.h2att.bias'], flat('attention.alpha_net.weight'), sd['attention.alpha_net.bias']
    xpre, fcrow = z(S, G), z(G)
    O.linear_fwd(xt, wa_ih[2 * R:], sd['att_lstm.bias_ih'], xpre, S, G, IE, ldw=Ka)
    O.linear_fwd(fc, wa_ih[R:], sd['att_lstm.bias_hh'], fcrow, 1, G, R, ldw=Ka)
    hl, cl, ca, lin = z(S + 1, R), z(S + 1, R), z(S + 1, R), z(S + 1, 2 * R)
    act_a, act_l, att_h, tanh, wgt, dots = z(S, G), z(S, G), z(S, AH), z(S, L, AH), z(S, L), z(S, 256)
    for i in range(S):
        O.topdown_cell_fwd(xpre[i], fcrow, None, [(hl[i], wa_ih, Ka, R), (lin[i][R:], wa_hh, R, R)], ca[i], ca[i + 1], lin[i + 1][R:], act_a[i], R)
        O.linear_fwd(lin[i + 1][R:], h2w, h2b, att_h[i], 1, AH, R)
        O.cap_att_dots_fwd(patt, att_h[i], aw, ab, L, AH, tanh[i], dots[i])
        O.cap_att_apply_fwd(att, dots[i], L, R, wgt[i], lin[i + 1])
        O.topdown_cell_fwd(None, sd['lang_lstm.bias_ih'], sd['lang_lstm.bias_hh'], [(lin[i + 1], wl_ih, 2 * R, 2 * R), (hl[i], wl_hh, R, R)],
                           cl[i], cl[i + 1], hl[i + 1], act_l[i], R)
    ta_ih, ta_hh, tl_ih, tl_hh, th2 = T('att_lstm.weight_ih'), T('att_lstm.weight_hh'), T('lang_lstm.weight_ih'), T('lang_lstm.weight_hh'), T('attention.h2att.weight')
    dga, dgl, dares, dwl, ddot, datt_h, dca, dcl = z(S, G), z(S, G), z(S, R), z(S, 256), z(S, L), z(S, AH), z(2, R), z(2, R)
    k = 0
    for i in range(S - 1, -1, -1):
        last = i == S - 1
        O.topdown_cell_bwd([] if last else [(dga[i + 1], ta_ih, G, G), (dgl[i + 1], tl_hh, G, G)], dout[i], None, None if last else dcl[k],
                           act_l[i], cl[i], cl[i + 1], dgl[i], dcl[1 - k], R)
        O.linear_fwd(dgl[i], tl_ih, None, dares[i], 1, R, G)
        O.linear_fwd(dares[i], att, None, dwl[i], 1, L, R)
        O.cap_att_bwd_step_centered(dwl[i], tanh[i], wgt[i], aw, L, AH, ddot[i], datt_h[i])
        O.topdown_cell_bwd([(dgl[i], tl_ih[R * G:], G, G), (datt_h[i], th2, AH, AH)] + ([] if last else [(dga[i + 1], ta_hh, G, G)]), None, None,
                           None if last else dca[k], act_a[i], ca[i], ca[i + 1], dga[i], dca[1 - k], R)
        k = 1 - k
    g = {n: torch.zeros_like(v) for n, v in sd.items()}
    dpatt, datt, dgsum, dfc, dX, X = z(L, AH), z(L, R), z(G), z(R), z(S, Ka), z(S, Ka)
    O.cap_attention_bwd_batched(ddot, wgt, None, R, tanh, aw, S, L, AH, dpatt, datt, g['attention.alpha_net.weight'], g['attention.alpha_net.bias'])
    O.linear_bwd_w(wgt, dares, datt, None, S, L, R)
    O.colsum(dga, S, G, G, dgsum)
    O.linear_fwd(dgsum, ta_ih[R * G:], None, dfc, 1, R, G)
    if S > 1:
        O.pack_rows(X[1:], Ka, hl[1:], R, S - 1, R)
    O.pack_rows(X[:, R:], Ka, fc, 0, S, R)
    O.pack_rows(X[:, 2 * R:], Ka, xt, IE, S, IE)
    O.linear_bwd_w(dga, X, g['att_lstm.weight_ih'], g['att_lstm.bias_ih'], S, G, Ka)
    O.linear_bwd_w(dga, lin[:, R:], g['att_lstm.weight_hh'], g['att_lstm.bias_hh'], S, G, R, ldx=2 * R)
    O.linear_bwd_w(dgl, lin[1:], g['lang_lstm.weight_ih'], g['lang_lstm.bias_ih'], S, G, 2 * R)
    O.linear_bwd_w(dgl, hl, g['lang_lstm.weight_hh'], g['lang_lstm.bias_hh'], S, G, R)
    O.linear_bwd_w(datt_h, lin[1:, R:], g['attention.h2att.weight'], g['attention.h2att.bias'], S, AH, R, ldx=2 * R)
    nws = O.linear_bwd_x_ws_floats(S, G, Ka)
    O.linear_bwd_x(dga, wa_ih, dX, S, G, Ka, ws=z(max(nws, 1)))
    torch.cuda.synchronize()
    g.update({'d xt': dX[:, 2 * R:], 'd fc': dfc, 'd att': datt, 'd p_att': dpatt})
    states = dict(h_att=lin[1:, R:], c_att=ca[1:], h_lang=hl[1:], c_lang=cl[1:])
    return states, g


@pytest.mark.parametrize('R,IE,AH,S', STEP_SHAPES + [(8, 10, 6, 2)])
def test_step_entries_vs_torch(R, IE, AH, S):
    """(8, 12, 8, 1): one partial workgroup, two live lanes, no recurrence, segment lengths all different (a wrong column offset shows);
    (8, 12, 8, 3): the recurrence; (260, 128, 64, 3): 65 workgroups, a ragged second trip of the float4 loop, rnn_size != att_hid_size;
    (512, 512, 512, 5): the product's size; (8, 10, 6, 2): leading dimension 26 and a 6-long segment, the scalar loop.
    h / c of both cells at every step and all gradients for a random d(output) per step against torch autograd."""
    O = ops()
    L = 10 if R == 8 else 196
    ref = core_reference(R, IE, AH, S, L, seed=R + IE + S)
    states, g = _run_core(O, ref, R, IE, AH, S, L)
    es = {k: rel_err(v, ref[k]) for k, v in states.items()}
    eg = grad_errs(g, ref['grads'])
    print('topdown steps R=%d IE=%d AH=%d S=%d: states %.2e  grads %.2e (%s)' % (R, IE, AH, S, max(es.values()), max(eg.values()), max(eg, key=eg.get)))
    assert set(eg) == set(ref['grads']) and len(eg) == 16
    for k, v in es.items():
        assert v < FWD_TOL, (k, v)
    for k, v in eg.items():
        assert v < GRAD_TOL, (k, v)


def test_step_entries_reject_bad_shapes_before_any_launch():
    from lang2seg_amd._lib import L2SError
    O = ops()
    buf = torch.full((4096,), 7.0, device=DEV)
    seg = (buf, buf, 8, 8)
    with pytest.raises(L2SError):
        O.topdown_cell_fwd(buf, None, None, [seg], buf, buf, buf, buf, 6)           # R % 4 != 0
    with pytest.raises(L2SError):
        O.topdown_cell_bwd([seg], None, None, None, buf, buf, buf, buf, buf, 6)
    with pytest.raises(L2SError):
        O.topdown_cell_fwd(buf, None, None, [(buf, buf, 4, 8)], buf, buf, buf, buf, 8)   # leading dimension shorter than the segment
    with pytest.raises(L2SError):
        O.cap_att_apply_fwd(buf, buf, 300, 8, buf, buf)                             # more than 256 locations
    torch.cuda.synchronize()
    assert bool((buf == 7.0).all())                                                 # nothing was launched


# ------------------------------------------------------------------ 2. the captioner in the network
_STEPS = {}


def _masks(opt, S, T, seed=41):
    g = torch.Generator().manual_seed(seed)
    mk = lambda *s: (torch.rand(*s, generator=g) > 0.5).float() / 0.5
    R, IE = opt['rnn_size'], opt['input_encoding_size']
    return dict(att=mk(196, R), fc=mk(R), xt=mk(S, IE), out=mk(S, R))


def _device_step(variant, with_masks, dtype):
    """one whole step of the tiny recipe (96x128 blob, 4 tokens, recorded sampling keys) with caption_model = 'topdown'; cached"""
    key = (variant, with_masks, dtype)
    if key not in _STEPS:
        from lang2seg_amd import selftest
        blob, over, ocfg, samp = edge_step_inputs()
        opt = td_opt()
        sd = make_sd(opt, seed=3, variant=variant)
        net = selftest.build_net(opt, over, dtype, sd, variant=variant)
        if dtype == 'bf16':
            # the f32 step's proposal list is forced into the bf16 step (bf16 scores reorder near-ties; the sampled RoIs must be the same)
            t32 = _device_step(variant, with_masks, 'f32')['net'].t
            n = int(t32['proposal_n'].item())
            samp = dict(samp, forced_proposals=(t32['proposal_rois'].cpu().numpy()[:n], t32['proposal_scores'].cpu().numpy()[:n]))
        net.parity = selftest.parity_from_samp(samp)
        dev = net.upload_blob(blob, 0)
        drops = _masks(opt, dev['S'], dev['T']) if with_masks else {}
        net.parity['drops'] = {k: v.to(DEV) for k, v in drops.items()}
        lv = net.forward_backward(dev).cpu().numpy()
        torch.cuda.synchronize()
        _STEPS[key] = dict(net=net, opt=opt, sd=sd, blob=blob, ocfg=ocfg, samp=samp, drops=drops, lv=lv)
    return _STEPS[key]


@pytest.mark.parametrize('with_masks', [False, True])
@pytest.mark.parametrize('variant', ['cycle', 'cycle_response'])
def test_network_step_vs_oracle_f32(variant, with_masks):
    """exact-f32 mode against the subclassed oracle on the device's own proposals: loss_caption and total_loss within 1e-4, fc_feats /
    att_feats forward, d(att_feats), d(fc_feats) and every caption_model.* gradient within 1e-4"""
    from oracle import weights as OW
    s = _device_step(variant, with_masks, 'f32')
    net, lv = s['net'], s['lv']
    n = int(net.t['proposal_n'].item())
    assert n > 0
    samp = dict(s['samp'], forced_proposals=(net.t['proposal_rois'].cpu().numpy()[:n], net.t['proposal_scores'].cpu().numpy()[:n]))
    onet = TopDownOracleNet(s['sd'], s['opt'], s['ocfg'], variant=variant)
    T, L = onet.forward_train(s['blob'], samp, s['drops'] or None)
    onet.backward()
    slots = dict(zip(OW.loss_keys(variant), net._loss_slots()))
    el = {k: abs(lv[slots[k]] - float(L[k])) / max(1.0, abs(float(L[k]))) for k in ('loss_caption', 'total_loss')}
    ef = dict(fc_feats=rel_err(net.t['fc_feats'], onet.t_fc), att_feats=rel_err(net.t['att_feats'], onet.t_att))
    ed = dict(d_att=rel_err(net.t['cap.datt'], onet.t_att.grad), d_fc=rel_err(net.t['cap.dfc'], onet.t_fc.grad))
    keys = [k for k in net.P.trainable if k.startswith(CAP)]
    dev_g = {k: net.P.view(k, net.P.grad) for k in keys}
    eg = grad_errs(dev_g, {k: onet.p[k].grad for k in keys})
    print('topdown %s%s f32 vs oracle: losses %.2e  feats %.2e  d(att) %.2e d(fc) %.2e  grads %.2e (%s)' % (
        variant, ' masks' if with_masks else '', max(el.values()), max(ef.values()), ed['d_att'], ed['d_fc'], max(eg.values()), max(eg, key=eg.get)))
    print('    ' + '  '.join('%s %.2e' % (k[len(CAP):], eg[k]) for k in sorted(eg, key=eg.get, reverse=True)[:4]))
    assert len(keys) == 21 and float(L['loss_caption']) > 0.1
    for k, v in el.items():
        assert np.isfinite(lv[slots[k]]) and v < LOSS_TOL, (k, v)
    bad = [(k, v) for k, v in list(ef.items()) + list(ed.items()) + list(eg.items()) if not v < GRAD_TOL]
    assert not bad, bad


@pytest.mark.parametrize('variant', ['cycle', 'cycle_response'])
def test_network_step_bf16_vs_f32(variant):
    """bf16 mode against the f32 device step of the same inputs and masks: losses within 1e-2; cosine >= 0.99 for every caption_model.*
    gradient, d(att_feats) and d(fc_feats).  (alpha_net.bias: its exact gradient is 0, see topdown_util.grad_errs - no direction to compare.)"""
    from oracle import weights as OW
    a, b = _device_step(variant, True, 'f32'), _device_step(variant, True, 'bf16')
    na, nb = a['net'], b['net']
    slots = dict(zip(OW.loss_keys(variant), na._loss_slots()))
    el = {k: abs(b['lv'][i] - a['lv'][i]) / max(1.0, abs(a['lv'][i])) for k, i in slots.items()}
    keys = [k for k in na.P.trainable if k.startswith(CAP) and not k.endswith('alpha_net.bias')]
    cs = {k: cosine(nb.P.view(k, nb.P.grad), na.P.view(k, na.P.grad)) for k in keys}
    cs['d_att'] = cosine(nb.t['cap.datt'].float(), na.t['cap.datt']); cs['d_fc'] = cosine(nb.t['cap.dfc'], na.t['cap.dfc'])
    print('topdown %s bf16 vs f32: losses %.2e  lowest cosine %.4f (%s)' % (variant, max(el.values()), min(cs.values()), min(cs, key=cs.get)))
    for k, v in el.items():
        assert v < BF16_LOSS_RTOL, (k, v)
    for k, v in cs.items():
        assert v >= BF16_COS, (k, v)


# ------------------------------------------------------------------ 3. the reference fixture on the device
def test_reference_fixture_through_the_device_captioner():
    """tests/golden/ref_topdown.npz (the reference's own TopDownModel, eval mode) through Network._caption_fwd / _caption_bwd: its
    log-probabilities, loss and the gradient of every parameter and of both feature inputs"""
    from lang2seg_amd import selftest
    z = np.load(GOLD)
    opt = td_opt(**{k[4:]: int(z[k]) for k in z.files if k.startswith('opt.')})
    net = selftest.build_net(opt, {}, 'f32', None, num_layers=50)
    net.load_state_dict({CAP + k[2:]: z[k] for k in z.files if k.startswith('w.')})
    net.eval()
    net.keep_logprobs, net.parity, net._cap_pre = True, None, None
    seq, masks = z['seq'], z['masks']
    S = int(z['logprobs'].shape[1])
    d = dict(S=S, cap_in=torch.from_numpy(seq[0, :S].copy()).to(DEV), cap_tgt=torch.from_numpy(seq[0, 1:S + 1].copy()).to(DEV),
             cap_mask=torch.from_numpy(masks[0, 1:S + 1].copy()).to(DEV))
    att = torch.from_numpy(z['att_feats'][0]).to(DEV).contiguous()
    net.t = {'fc_feats': torch.from_numpy(z['fc_feats'][0]).to(DEV).contiguous()}
    loss = torch.zeros(8, device=DEV)
    net.P.grad.zero_()
    net._caption_fwd(d, att, loss)
    datt = net._caption_bwd(d, att)
    net.join_wgrad()                                                            # att_embed's weight gradient is a queued convolution weight gradient
    for f in net._cap_deferred:
        f()
    torch.cuda.synchronize()
    e_lp, e_loss = rel_err(net.t['cap.logp'], z['logprobs'][0]), abs(float(loss[5]) - float(z['loss'])) / max(1.0, abs(float(z['loss'])))
    ref_g = {CAP + k[2:]: z[k] for k in z.files if k.startswith('g.')}
    eg = grad_errs({k: net.P.view(k, net.P.grad) for k in ref_g}, ref_g)
    eg['d att_feats'] = rel_err(datt, z['g_att_feats'][0]); eg['d fc_feats'] = rel_err(net.t['cap.dfc'], z['g_fc_feats'][0])
    print('topdown fixture on the device: logprobs %.2e loss %.2e grads %.2e (%s)' % (e_lp, e_loss, max(eg.values()), max(eg, key=eg.get)))
    assert e_lp < FWD_TOL and e_loss < LOSS_TOL
    assert len(ref_g) == 21
    for k, v in eg.items():
        assert v < GRAD_TOL, (k, v)


# ------------------------------------------------------------------ 4. launch tape and snapshot restore
def _tape_net(opt, sd, over, tape):
    from lang2seg_amd import selftest
    from lang2seg_amd.optim import SGD
    net = selftest.build_net(opt, over, 'f32', sd)
    net.use_tape = tape
    return net, SGD(net, 0.0, keep_grad=True)          # lr 0: the weights stay put, the steps differ by their dropout masks and sampling keys


def test_tape_replay_equals_eager_topdown():
    """three whole topdown steps with the production RNG (all four captioner dropouts on, sampling keys from the device counter): replayed
    from the launch tape they equal the eagerly issued steps bit for bit - the whole gradient buffer after every step - and a second
    eager run gives the same bits again; the loss scalars (float atomics) within 1e-5"""
    blob, over, ocfg, samp = edge_step_inputs()
    opt = td_opt()
    sd = make_sd(opt, seed=3)
    res = []
    for tape in (False, True, False):
        net, sgd = _tape_net(opt, sd, over, tape)
        steps = []
        for _ in range(3):
            lv = net.train_step(dict(blob), 0, sgd)
            torch.cuda.synchronize()
            steps.append((np.asarray(lv), net.P.grad.clone()))
        if tape:
            assert len(net._tapes) == 1
        res.append(steps)
    P = net.P
    cap_lo = min(P.offsets[k] for k in P.trainable if k.startswith(CAP + 'core.'))
    cap_hi = max(P.offsets[k] + int(np.prod(P.shapes[k])) for k in P.trainable if k.startswith(CAP + 'core.'))
    for s_, (a, b, c) in enumerate(zip(*res)):
        assert float(a[1][cap_lo:cap_hi].abs().max()) > 0
        assert torch.equal(a[1], b[1]), ('tape vs eager', s_, int((a[1] != b[1]).sum()))
        assert torch.equal(a[1], c[1]), ('run vs run', s_, int((a[1] != c[1]).sum()))
        assert np.allclose(a[0], b[0], rtol=1e-5, atol=1e-6) and np.allclose(a[0], c[0], rtol=1e-5, atol=1e-6), (s_, a[0], b[0], c[0])
    assert not torch.equal(res[0][0][1][cap_lo:cap_hi], res[0][1][1][cap_lo:cap_hi])      # the dropout masks did change between steps


def test_snapshot_restore_and_mismatch_topdown(tmp_path):
    """SolverWrapper.snapshot of a topdown network after one real update, restored into a fresh network: every tensor the same bits, and
    so is the next step's whole gradient buffer; loading the file into a default (att2in2) network is an error naming --caption_model"""
    from lang2seg_amd import selftest
    from lang2seg_amd.loaders.synthetic_loader import SyntheticLoader
    from lang2seg_amd.model.train_val import SolverWrapper
    from lang2seg_amd.optim import SGD
    blob, over, ocfg, samp = edge_step_inputs()
    opt = td_opt()
    sd = make_sd(opt, seed=3)
    ld = SyntheticLoader(num_images=2, H=32, W=32, T=3, vocab_size=10)
    a = selftest.build_net(opt, over, 'f32', sd)
    a.parity = selftest.parity_from_samp(samp)
    a.forward_backward(a.upload_blob(blob, 0))
    SGD(a, 1e-2).step()
    torch.cuda.synchronize()
    sfile, nfile = SolverWrapper(a, ld, str(tmp_path / 'out'), str(tmp_path / 'tb')).snapshot(7)
    b = selftest.build_net(opt, over, 'f32', None)
    assert SolverWrapper(b, ld, str(tmp_path / 'out'), str(tmp_path / 'tb')).from_snapshot(sfile, nfile) == 7
    sa, sb = a.state_dict(), b.state_dict()
    assert set(sa) == set(sb) and all(torch.equal(sa[k], sb[k]) for k in sa)
    assert any(not np.array_equal(sa[k].numpy(), sd[k]) for k in sa if k.startswith(CAP + 'core.'))
    b.parity = selftest.parity_from_samp(samp)
    b.train()
    la = a.forward_backward(a.upload_blob(blob, 0)).cpu().numpy()
    lb = b.forward_backward(b.upload_blob(blob, 0)).cpu().numpy()
    torch.cuda.synchronize()
    assert float(a.P.grad.abs().max()) > 0
    assert torch.equal(a.P.grad, b.P.grad), int((a.P.grad != b.P.grad).sum())
    assert np.allclose(la, lb, rtol=1e-5, atol=1e-6), (la, lb)
    other = selftest.build_net(dict(opt, caption_model='att2in2'), over, 'f32', None)
    with pytest.raises(ValueError, match='--caption_model topdown'):
        SolverWrapper(other, ld, str(tmp_path / 'out'), str(tmp_path / 'tb')).from_snapshot(sfile, nfile)
    with pytest.raises(ValueError, match='--caption_model topdown'):
        other.load_state_dict(torch.load(sfile, map_location='cpu'))


def test_forward_only_summary_and_mixed_shapes_topdown():
    """get_summary (forward only) between steps, and steps of two image sizes / token counts through the tape: finite losses, and the
    replayed step after the detour equals the same sequence issued eagerly on a second network bit for bit"""
    from oracle import synth as OS
    blob, over, ocfg, samp = edge_step_inputs()
    blob2 = OS.make_blob(112, 96, 2, 60, seed=29)
    opt = td_opt()
    sd = make_sd(opt, seed=3)
    a, sa = _tape_net(opt, sd, over, True)
    b, sb = _tape_net(opt, sd, over, False)
    la, lb = [], []
    for net, sgd, out in ((a, sa, la), (b, sb, lb)):
        out += [net.train_step(dict(blob), 0, sgd), net.train_step(dict(blob2), 0, sgd)]
        net.get_summary(dict(blob), 0)
        out.append(net.train_step(dict(blob), 0, sgd))
    torch.cuda.synchronize()
    assert all(np.isfinite(np.asarray(l)).all() for l in la + lb)
    assert len(a._tapes) == 2
    assert torch.equal(a.P.grad, b.P.grad), int((a.P.grad != b.P.grad).sum())


# ------------------------------------------------------------------ 5. the default captioner is what it was
# recorded on the parent commit with this very function (tiny default step: 160x224 blob, 6 tokens, f32, production RNG): launches on the
# tape and the reported losses with the plain optimiser, the SHA-1 of the whole gradient buffer with an optimiser that keeps the gradients
# (it adds three clears to the tape: 476 / 239 launches)
PARENT_LAUNCHES = {'cycle': 473, 'vgg': 236}
PARENT_LOSSES = {'cycle': '0x1.0cd304p-1 0x1.65a62p-6 0x1.2b53a4p+2 0x1.fb1ba2p-13 0x1.55aef6p-1 0x1.18fe2p+2 0x1.4905dp+3',
                 'vgg': '0x1.7930dcp+1 0x1.0d3e1p-3 0x1.230752p+4 0x1.1563e8p-4 0x1.a14016p-1 0x1.62674ep+4'}
PARENT_KEEP = {'cycle': (476, '614f46d67bcc0f576f7b976055252fdfa02abd16'), 'vgg': (239, '9fe81a2b049a71f764701e03878e24d058bc60f3')}


def default_step_record(variant, keep, opt_over=None, net_over=None):
    """the tiny default step of __graft_entry__.smoke() (att2in2; production RNG from the device counter, as the tape needs) recorded on a
    launch tape -> (launches, sha1 of the gradient buffer, losses).  opt_over: options that differ from the default (an encoder or a
    captioner other than the default takes its weights from a seeded torch module, as the suites of those paths do); net_over: Network
    attributes set before the step (cap_persistent, cap_projected)"""
    from lang2seg_amd import selftest, ops as O
    from lang2seg_amd.optim import SGD
    from oracle import weights as OW, synth as OS
    import rnn_encoder_util
    opt = OW.default_opt(vocab_size=60, seq_length=6)
    if variant == 'vgg':
        opt['C4_feat_dim'] = 512
    opt.update(opt_over or {})
    if opt.get('caption_model') == 'topdown':
        sd = make_sd(opt, seed=3, variant=variant)
    elif opt.get('caption_model') in ('adaatt', 'adaattmo'):
        import adaatt_util
        sd = adaatt_util.make_sd(opt, seed=3, variant=variant)
    elif 'rnn_type' in (opt_over or {}):
        sd = rnn_encoder_util.make_sd(opt, seed=3, variant=variant)
    else:
        sd = OW.make_state_dict(opt, seed=3, head_gain=4.0, variant=variant)
    blob = OS.make_blob(160, 224, 6, 60, seed=5)
    over = dict(BATCH_SIZE=16, RPN_PRE_NMS_TOP_N=600, RPN_POST_NMS_TOP_N=100, RPN_BATCHSIZE=64)
    net = selftest.build_net(opt, over, 'f32', sd, variant=variant)
    for k, v in (net_over or {}).items():
        assert hasattr(net, k), k
        setattr(net, k, v)
    net.use_tape = True
    lv = np.asarray(net.train_step(dict(blob), 0, SGD(net, 0.0, keep_grad=True) if keep else SGD(net, 1e-4)), dtype=np.float32)
    torch.cuda.synchronize()
    (h, _, _, _), = net._tapes.values()
    return int(O.tape_size(h)), hashlib.sha1(net.P.grad.cpu().numpy().tobytes()).hexdigest(), lv


@pytest.mark.parametrize('variant', ['cycle', 'vgg'])
def test_default_captioner_issues_the_parents_launches(variant):
    """--caption_model att2in2 (the default) issues exactly the launches of the parent commit - 473 on the ResNet cycle network, 236 on
    VGG16 - and reports its losses (scalars summed with float atomics: to 1e-6)"""
    n, _, lv = default_step_record(variant, keep=False)
    print('default step %s: %d launches, losses %s' % (variant, n, ' '.join(float(v).hex() for v in lv)))
    assert n == PARENT_LAUNCHES[variant]
    ref = np.array([float.fromhex(v) for v in PARENT_LOSSES[variant].split()], dtype=np.float32)
    assert np.allclose(lv, ref, rtol=1e-6, atol=0), (lv, ref)


@pytest.mark.parametrize('variant', ['cycle', 'vgg'])
def test_default_captioner_computes_the_parents_bits(variant):
    """the whole gradient buffer of that step (kept by the optimiser) has the parent commit's SHA-1"""
    n, sha, _ = default_step_record(variant, keep=True)
    print('default step %s, gradients kept: %d launches, grad sha1 %s' % (variant, n, sha))
    assert (n, sha) == PARENT_KEEP[variant]


# every other recurrent path (cycle network), recorded in the same way, twice per configuration with equal results, before the step kernels
# were gathered over csrc/recur.h: name -> (option overrides, Network attribute overrides), and (launches, SHA-1, losses) with the gradients kept
RECURRENT_PATHS = {
    'per_token': ({}, dict(cap_persistent=False)),
    'unprojected': ({}, dict(cap_persistent=False, cap_projected=False)),
    'topdown': (dict(caption_model='topdown'), {}),
    'adaatt': (dict(caption_model='adaatt', adaatt=1), {}),
    'adaattmo': (dict(caption_model='adaattmo', adaatt=1), {}),
    'gru2_bi': (dict(rnn_type='gru', rnn_num_layers=2, bidirectional=1), {}),
    'rnn1_uni': (dict(rnn_type='rnn', rnn_num_layers=1, bidirectional=0), {}),
    'lstm2_uni': (dict(rnn_type='lstm', rnn_num_layers=2, bidirectional=0), {}),
}
PARENT_PATHS = {
    'adaatt': (545, '23c378d91bc357fa81cd30862d67b3927e55dc74',
        '0x1.0cd304p-1 0x1.65a62p-6 0x1.2b53a4p+2 0x1.fb1ba2p-13 0x1.55aef6p-1 0x1.079eb8p+2 0x1.40561cp+3'),
    'adaattmo': (545, '26a271a51d63d0b95e9907ef7ab7239f261b2ee2',
        '0x1.0cd304p-1 0x1.65a62p-6 0x1.2b53a4p+2 0x1.fb1ba2p-13 0x1.55aef6p-1 0x1.0505f4p+2 0x1.3f09b8p+3'),
    'gru2_bi': (502, '7de52a4f54feac7f0dc17fff5d85c0165ccf1fbe',
        '0x1.64136cp+0 0x1.7c9a62p-5 0x1.3645b6p+2 0x1.5d2148p-12 0x1.6f365p-1 0x1.1b4324p+2 0x1.6db994p+3'),
    'lstm2_uni': (492, '480aefbd69b27ca8ac0ad300543553929af9e345',
        '0x1.71fed2p-1 0x1.42c196p-6 0x1.31ca16p+2 0x1.47c584p-13 0x1.4d8054p-1 0x1.19492ap+2 0x1.52243cp+3'),
    'per_token': (516, '122a8af3bcc3ba05dd47ea7f16350be7eaa9030f',
        '0x1.0cd304p-1 0x1.65a62p-6 0x1.2b53a4p+2 0x1.fb1ba2p-13 0x1.55aef6p-1 0x1.18fe2p+2 0x1.4905dp+3'),
    'rnn1_uni': (468, '83ea4f5279396975d2ed4a6564c17c9515a2b6b2',
        '0x1.7d759p+1 0x1.327b74p-2 0x1.215cdcp+2 0x1.3f26fcp-8 0x1.2651aap+0 0x1.143d2p+2 0x1.a8b058p+3'),
    'topdown': (563, 'ba6d290d178b164bcbe0e106635f2fdd10fe2e7b',
        '0x1.0cd304p-1 0x1.65a62p-6 0x1.2b53a4p+2 0x1.fb1ba2p-13 0x1.55aef6p-1 0x1.06d3c6p+2 0x1.3ff0a2p+3'),
    'unprojected': (526, 'bab2ec9385ce1d0f9b38bf9ae7f5ac398bdfb6f8',
        '0x1.0cd304p-1 0x1.65a62p-6 0x1.2b53a4p+2 0x1.fb1ba2p-13 0x1.55aef6p-1 0x1.18fe2p+2 0x1.4905dp+3'),
}


@pytest.mark.parametrize('name', sorted(RECURRENT_PATHS))
def test_recurrent_paths_compute_the_parents_bits(name):
    """the per-token att2in2 kernels (projected and unprojected), the top-down and AdaAtt captioners and the GRU / tanh-RNN / stacked LSTM encoders:
    launches, the SHA-1 of the whole gradient buffer and the losses (to 1e-6) of the tiny step are the parent commit's"""
    opt_over, net_over = RECURRENT_PATHS[name]
    n, sha, lv = default_step_record('cycle', True, opt_over, net_over)
    print('%s: %d launches, grad sha1 %s, losses %s' % (name, n, sha, ' '.join(float(v).hex() for v in lv)))
    pn, psha, plosses = PARENT_PATHS[name]
    assert (n, sha) == (pn, psha)
    ref = np.array([float.fromhex(v) for v in plosses.split()], dtype=np.float32)
    assert np.allclose(lv, ref, rtol=1e-6, atol=0), (lv, ref)


# ------------------------------------------------------------------ 6. strict load
def test_state_dict_loads_key_for_key():
    """a state_dict() of the restatement loads under caption_model., and the network's state_dict() returns the same keys, shapes and values"""
    from lang2seg_amd import selftest
    opt = td_opt()
    torch.manual_seed(9)
    mod = TopDownRef(opt)
    net = selftest.build_net(opt, {}, 'f32', None)
    net.load_state_dict({CAP + k: v for k, v in mod.state_dict().items()}, strict=False)
    out = {k: v for k, v in net.state_dict().items() if k.startswith(CAP)}
    want = {CAP + k: v for k, v in mod.state_dict().items()}
    assert list(out) == list(want)
    for k, v in want.items():
        assert tuple(out[k].shape) == tuple(v.shape) and torch.equal(out[k], v.detach()), k
