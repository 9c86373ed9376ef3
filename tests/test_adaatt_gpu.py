"""The adaptive-attention captioners on the device (csrc/adaatt_step.hip, nets/adaatt.py and nets/captioners.py AdaAtt) against the torch
restatement of tests/adaatt_util.py, which tests/test_adaatt_cpu.py pins to the reference's own models.
Bounds: the kernel family's (tests/test_kernels_gpu.py rel_err) 1e-5 forward and 1e-4 gradients; 1e-4 on losses in exact-f32 mode; bf16:
losses within 1e-2 and cosine >= 0.99 per gradient tensor against the f32 device step.

Worst values measured on an MI355X (this file's own prints):
  step entries, ten cases      h / c / fake / out 4.0e-07, gradients 1.7e-06 (attention.fr_embed.bias), the locations' sum (ctx2att.bias) 7.2e-07
  network vs oracle, f32       losses 2.3e-07, fc / att features 1.4e-06, d(att_feats) 7.8e-07, d(fc_feats) 3.6e-07; captioner gradients
                               adaatt 2.1e-06 (cycle), 1.7e-06 (cycle, masks), 3.1e-06 (cycle_response), 2.8e-06 (cycle_response, masks);
                               adaattmo 1.8e-06, 1.3e-06, 6.0e-06 (alpha_net.weight), 2.0e-06
  network bf16 vs f32          losses 1.5e-03, lowest cosine 0.9977 (d(att_feats), adaattmo cycle_response)
  reference fixtures           log-probabilities 1.5e-07, loss 7.9e-08, gradients 5.8e-06 (adaatt, ctx2att.bias), 8.4e-07 (adaattmo)

The sums over the slots that cancel (d(hoe), and through it ho_embed.* / ho_linear.*; ctx2att.bias) are taken about their PI-weighted mean by
l2s_adaatt_att_bwd_step, as l2s_cap_att_bwd_step_centered does for the top-down captioner; the oracle evaluates its captioner in float64."""
import os

import numpy as np
import pytest
import torch

from rnn_encoder_util import edge_step_inputs
from adaatt_util import (CAP, GATES, STEP_SHAPES, AdaAttRef, AdaAttOracleNet, core_reference, rel_err, grad_errs, cosine, ada_opt, make_sd,
                         make_masks)

pytestmark = pytest.mark.gpu

DEV = 'cuda'
FWD_TOL, GRAD_TOL, LOSS_TOL = 1e-5, 1e-4, 1e-4
BF16_LOSS_RTOL, BF16_COS = 1e-2, 0.99
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODELS = ['adaatt', 'adaattmo']
OTHER = {'adaatt': 'adaattmo', 'adaattmo': 'adaatt'}


def ops():
    from lang2seg_amd import ops as O
    return O


# ------------------------------------------------------------------ 1. the step entries alone
def _run_core(O, ref, model, R, L, S):
    """the core through nets/adaatt.py's sequence of launches on plain tensors; returns the per-step states and the gradients under the
    restatement's names"""
    from lang2seg_amd.nets import adaatt as AA
    G = GATES[model]
    W = (G + 1) * R
    f = lambda t: t.detach().float().to(DEV).contiguous()
    sd = {k: f(v) for k, v in ref['core'].state_dict().items()}
    g = {k: torch.zeros_like(v) for k, v in sd.items()}
    pv, gv = (lambda k: sd[k].view(-1)), (lambda k: g[k].view(-1))
    z = lambda *s: torch.zeros(*s, device=DEV)
    xt, fc, att, patt, dout = (f(ref[k]) for k in ('xt', 'fc', 'att', 'p_att', 'dout'))
    masks = {k: f(v) for k, v in ref['drops'].items()}
    xpre, fcrow = z(S, W), z(W)
    O.linear_fwd(xt, pv('lstm.w2h.weight'), pv('lstm.w2h.bias'), xpre, S, G * R, R, ldy=W)
    O.linear_fwd(xt, pv('lstm.r_w2h.weight'), pv('lstm.r_w2h.bias'), xpre[:, G * R:], S, R, R, ldy=W)
    O.linear_fwd(fc, pv('lstm.v2h.weight'), pv('lstm.v2h.bias'), fcrow, 1, G * R, R)
    O.linear_fwd(fc, pv('lstm.r_v2h.weight'), pv('lstm.r_v2h.bias'), fcrow[G * R:], 1, R, R)
    B = {k: z(*shp) for k, shp in AA.fwd_shapes(S, L, R).items()}
    V = AA.core_fwd(O, pv, B, xpre, fcrow, att, patt, masks, S, L, R, G)
    torch.cuda.synchronize()
    states = dict(h=B['hs'][1:].clone(), c=B['cs'][1:].clone(), fake=B['fake'].clone(), out=B['outs'].clone())

    def bwd_x(dy, k, dx, M, accumulate=False, lddy=None, mul=None):
        N, K = sd[k].shape
        O.linear_bwd_x(dy, pv(k), dx, M, N, K, accumulate=accumulate, lddy=lddy, mul=mul, ws=z(max(O.linear_bwd_x_ws_floats(M, N, K), 1)))
    D = {k: z(*shp) for k, shp in AA.bwd_shapes(S, L, R, G).items()}
    wT = (sd['lstm.h2h.0.weight'].t().contiguous().view(-1), sd['lstm.r_h2h.weight'].t().contiguous().view(-1))
    dpatt, datt, dgsum, dfc, dxt = z(L, R), z(L, R), z(W), z(R), z(S, R)
    AA.core_bwd(O, pv, wT, bwd_x, B, D, V, dout, att, dpatt, datt, gv('attention.alpha_net.weight'), masks, S, L, R, G)
    O.colsum(D['dall'], S, W, W, dgsum)
    bwd_x(dgsum, 'lstm.v2h.weight', dfc, 1)
    bwd_x(dgsum[G * R:], 'lstm.r_v2h.weight', dfc, 1, accumulate=True)
    AA.core_wgrads(O, gv, B, D, V, dout, xt, fc, dgsum, S, R, R, G)
    bwd_x(D['dall'], 'lstm.w2h.weight', dxt, S, lddy=W)
    bwd_x(D['dall'][:, G * R:], 'lstm.r_w2h.weight', dxt, S, accumulate=True, lddy=W)
    torch.cuda.synchronize()
    g.update({'d xt': dxt, 'd fc': dfc, 'd att': datt, 'd p_att': dpatt})
    # what the step kernel says about the locations' sum (ctx2att.bias's gradient in the network) against the column sums of d(p_att)
    states['dctx'] = D['dctx'].sum(0)
    return states, g


@pytest.mark.parametrize('R,L,S,masks', [s + (False,) for s in STEP_SHAPES] + [(8, 10, 3, True)])
@pytest.mark.parametrize('model', MODELS)
def test_step_entries_vs_torch(model, R, L, S, masks):
    """(8, 10, 1): one partial workgroup, no recurrence, 11 slots; (8, 10, 3): the recurrence; (260, 196, 3): 65 workgroups, a ragged second
    trip of the float4 loop, 197 slots in a 256-thread softmax; (512, 196, 5): the product's size; (8, 10, 3) also with all five new masks.
    h / c / fake and the output at every step and all gradients for a random d(out) per step against torch autograd (float64)."""
    O = ops()
    ref = core_reference(model, R, L, S, seed=R + L + S, masks=masks)
    states, g = _run_core(O, ref, model, R, L, S)
    dctx = states.pop('dctx')
    es = {k: rel_err(v, ref[k]) for k, v in states.items()}
    eg = grad_errs(g, ref['grads'])
    e_ctx = rel_err(dctx, ref['grads']['d p_att'].sum(0))
    print('%s steps R=%d L=%d S=%d%s: states %.2e  grads %.2e (%s)  locations\' sum %.2e' % (
        model, R, L, S, ' masks' if masks else '', max(es.values()), max(eg.values()), max(eg, key=eg.get), e_ctx))
    assert set(eg) == set(ref['grads']) and len(eg) == 28
    for k, v in es.items():
        assert v < FWD_TOL, (k, v)
    for k, v in eg.items():
        assert v < GRAD_TOL, (k, v)
    assert e_ctx < GRAD_TOL


def test_step_entries_reject_bad_shapes_before_any_launch():
    from lang2seg_amd._lib import L2SError
    O = ops()
    buf = torch.full((1 << 16,), 7.0, device=DEV)
    cf = lambda R, G, **kw: O.adaatt_cell_fwd(buf, buf, buf, buf, buf, buf, buf, buf, buf, buf, buf, buf, R, G, **kw)
    cb = lambda R, G, **kw: O.adaatt_cell_bwd(buf, buf, buf, buf, buf, buf, buf, buf, buf, buf, R, G, **kw)
    for bad in (lambda: cf(6, 4), lambda: cb(6, 5),                               # R % 4 != 0
                lambda: cf(8, 3), lambda: cb(8, 6),                               # neither 4 nor 5 row blocks
                lambda: cf(8, 4, ld_hh=4), lambda: cf(8, 5, ld_r=4),              # a leading dimension shorter than its row
                lambda: cb(8, 4, ld_thh=24), lambda: cb(8, 5, ld_tr=4),
                lambda: O.adaatt_att_fwd(buf, buf, buf, buf, buf, buf, buf, buf, None, 2, 256, 8, buf, buf, buf, buf),        # L + 1 > 256
                lambda: O.adaatt_att_bwd_step(buf, buf, buf, buf, None, buf, buf, 2, 256, 8, buf, buf, buf, buf, buf, buf),
                lambda: O.adaatt_att_bwd_step(buf, buf, buf, buf, None, buf, buf, 2, 10, 6, buf, buf, buf, buf, buf, buf),    # R % 4 != 0
                lambda: O.adaatt_att_bwd_batched(buf, buf, buf, buf, None, buf, 2, 256, 8, buf, buf, buf)):
        with pytest.raises(L2SError):
            bad()
    torch.cuda.synchronize()
    assert bool((buf == 7.0).all())                                                 # nothing was launched


# ------------------------------------------------------------------ 2. the captioner in the network
_STEPS = {}


def _device_step(model, variant, with_masks, dtype):
    """one whole step of the tiny recipe (96x128 blob, 4 tokens, recorded sampling keys) with caption_model = model; cached"""
    key = (model, variant, with_masks, dtype)
    if key not in _STEPS:
        from lang2seg_amd import selftest
        blob, over, ocfg, samp = edge_step_inputs()
        opt = ada_opt(model)
        sd = make_sd(opt, seed=3, variant=variant)
        net = selftest.build_net(opt, over, dtype, sd, variant=variant)
        if dtype == 'bf16':
            # the f32 step's proposal list is forced into the bf16 step (bf16 scores reorder near-ties; the sampled RoIs must be the same)
            t32 = _device_step(model, variant, with_masks, 'f32')['net'].t
            n = int(t32['proposal_n'].item())
            samp = dict(samp, forced_proposals=(t32['proposal_rois'].cpu().numpy()[:n], t32['proposal_scores'].cpu().numpy()[:n]))
        net.parity = selftest.parity_from_samp(samp)
        dev = net.upload_blob(blob, 0)
        drops = make_masks(opt, dev['S']) if with_masks else {}
        net.parity['drops'] = {k: v.to(DEV) for k, v in drops.items()}
        lv = net.forward_backward(dev).cpu().numpy()
        torch.cuda.synchronize()
        _STEPS[key] = dict(net=net, opt=opt, sd=sd, blob=blob, ocfg=ocfg, samp=samp, drops=drops, lv=lv)
    return _STEPS[key]


@pytest.mark.parametrize('with_masks', [False, True])
@pytest.mark.parametrize('variant', ['cycle', 'cycle_response'])
@pytest.mark.parametrize('model', MODELS)
def test_network_step_vs_oracle_f32(model, variant, with_masks):
    """exact-f32 mode against the subclassed oracle on the device's own proposals: loss_caption and total_loss within 1e-4, fc_feats /
    att_feats forward, d(att_feats), d(fc_feats) and every caption_model.* gradient (33 keys) within 1e-4"""
    from oracle import weights as OW
    s = _device_step(model, variant, with_masks, 'f32')
    net, lv = s['net'], s['lv']
    n = int(net.t['proposal_n'].item())
    assert n > 0
    samp = dict(s['samp'], forced_proposals=(net.t['proposal_rois'].cpu().numpy()[:n], net.t['proposal_scores'].cpu().numpy()[:n]))
    onet = AdaAttOracleNet(s['sd'], s['opt'], s['ocfg'], variant=variant)
    T, L = onet.forward_train(s['blob'], samp, s['drops'] or None)
    onet.backward()
    slots = dict(zip(OW.loss_keys(variant), net._loss_slots()))
    el = {k: abs(lv[slots[k]] - float(L[k])) / max(1.0, abs(float(L[k]))) for k in ('loss_caption', 'total_loss')}
    ef = dict(fc_feats=rel_err(net.t['fc_feats'], onet.t_fc), att_feats=rel_err(net.t['att_feats'], onet.t_att))
    ed = dict(d_att=rel_err(net.t['cap.datt'], onet.t_att.grad), d_fc=rel_err(net.t['cap.dfc'], onet.t_fc.grad))
    keys = [k for k in net.P.trainable if k.startswith(CAP)]
    dev_g = {k: net.P.view(k, net.P.grad) for k in keys}
    eg = grad_errs(dev_g, {k: onet.p[k].grad for k in keys})
    print('%s %s%s f32 vs oracle: losses %.2e  feats %.2e  d(att) %.2e d(fc) %.2e  grads %.2e (%s)' % (
        model, variant, ' masks' if with_masks else '', max(el.values()), max(ef.values()), ed['d_att'], ed['d_fc'], max(eg.values()), max(eg, key=eg.get)))
    print('    ' + '  '.join('%s %.2e' % (k[len(CAP):], eg[k]) for k in sorted(eg, key=eg.get, reverse=True)[:4]))
    assert len(keys) == 33 and float(L['loss_caption']) > 0.1
    for k, v in el.items():
        assert np.isfinite(lv[slots[k]]) and v < LOSS_TOL, (k, v)
    bad = [(k, v) for k, v in list(ef.items()) + list(ed.items()) + list(eg.items()) if not v < GRAD_TOL]
    assert not bad, bad


@pytest.mark.parametrize('variant', ['cycle', 'cycle_response'])
@pytest.mark.parametrize('model', MODELS)
def test_network_step_bf16_vs_f32(model, variant):
    """bf16 mode against the f32 device step of the same inputs and masks (the f32 proposals forced): losses within 1e-2; cosine >= 0.99 for
    every caption_model.* gradient, d(att_feats) and d(fc_feats).  (alpha_net.bias: its exact gradient is 0 - no direction to compare.)"""
    from oracle import weights as OW
    a, b = _device_step(model, variant, True, 'f32'), _device_step(model, variant, True, 'bf16')
    na, nb = a['net'], b['net']
    slots = dict(zip(OW.loss_keys(variant), na._loss_slots()))
    el = {k: abs(b['lv'][i] - a['lv'][i]) / max(1.0, abs(a['lv'][i])) for k, i in slots.items()}
    keys = [k for k in na.P.trainable if k.startswith(CAP) and not k.endswith('alpha_net.bias')]
    cs = {k: cosine(nb.P.view(k, nb.P.grad), na.P.view(k, na.P.grad)) for k in keys}
    cs['d_att'] = cosine(nb.t['cap.datt'].float(), na.t['cap.datt']); cs['d_fc'] = cosine(nb.t['cap.dfc'], na.t['cap.dfc'])
    print('%s %s bf16 vs f32: losses %.2e  lowest cosine %.4f (%s)' % (model, variant, max(el.values()), min(cs.values()), min(cs, key=cs.get)))
    for k, v in el.items():
        assert v < BF16_LOSS_RTOL, (k, v)
    for k, v in cs.items():
        assert v >= BF16_COS, (k, v)


# ------------------------------------------------------------------ 3. the reference fixtures on the device
@pytest.mark.parametrize('model', MODELS)
def test_reference_fixture_through_the_device_captioner(model):
    """tests/golden/ref_<model>.npz (the reference's own model, eval mode) through Network._caption_fwd / _caption_bwd: its log-probabilities,
    loss and the gradient of every parameter and of both feature inputs"""
    from lang2seg_amd import selftest
    z = np.load(os.path.join(ROOT, 'tests', 'golden', 'ref_%s.npz' % model))
    opt = ada_opt(model, **{k[4:]: int(z[k]) for k in z.files if k.startswith('opt.')})
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
    print('%s fixture on the device: logprobs %.2e loss %.2e grads %.2e (%s)' % (model, e_lp, e_loss, max(eg.values()), max(eg, key=eg.get)))
    assert S == 6 and e_lp < FWD_TOL and e_loss < LOSS_TOL
    assert len(ref_g) == 33
    for k, v in eg.items():
        assert v < GRAD_TOL, (k, v)


# ------------------------------------------------------------------ 4. launch tape and snapshot restore
def _tape_net(opt, sd, over, tape):
    from lang2seg_amd import selftest
    from lang2seg_amd.optim import SGD
    net = selftest.build_net(opt, over, 'f32', sd)
    net.use_tape = tape
    return net, SGD(net, 0.0, keep_grad=True)          # lr 0: the weights stay put, the steps differ by their dropout masks and sampling keys


@pytest.mark.parametrize('model', MODELS)
def test_tape_replay_equals_eager(model):
    """three whole steps with the production RNG (all nine captioner dropouts on, sampling keys from the device counter): replayed from the
    launch tape they equal the eagerly issued steps bit for bit - the whole gradient buffer after every step - and a second eager run
    gives the same bits again; the loss scalars (float atomics) within 1e-5.  The masks did change between steps."""
    blob, over, ocfg, samp = edge_step_inputs()
    opt = ada_opt(model)
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


@pytest.mark.parametrize('model', MODELS)
def test_snapshot_restore_and_mismatch(model, tmp_path):
    """SolverWrapper.snapshot after one real update, restored into a fresh network: every tensor the same bits, and so is the next step's
    whole gradient buffer; an att2in2, a topdown and the OTHER AdaAtt network refuse the file with an error naming --caption_model"""
    from lang2seg_amd import selftest
    from lang2seg_amd.loaders.synthetic_loader import SyntheticLoader
    from lang2seg_amd.model.train_val import SolverWrapper
    from lang2seg_amd.optim import SGD
    blob, over, ocfg, samp = edge_step_inputs()
    opt = ada_opt(model)
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
    for o in ('att2in2', 'topdown', OTHER[model]):
        other = selftest.build_net(dict(opt, caption_model=o), over, 'f32', None)
        with pytest.raises(ValueError, match=r'--caption_model %s \(this network: %s\)' % (model, o)):
            SolverWrapper(other, ld, str(tmp_path / 'out'), str(tmp_path / 'tb')).from_snapshot(sfile, nfile)
        with pytest.raises(ValueError, match=r'--caption_model %s \(this network: %s\)' % (model, o)):
            other.load_state_dict(torch.load(sfile, map_location='cpu'))


@pytest.mark.parametrize('model', MODELS)
def test_forward_only_summary_and_mixed_shapes(model):
    """get_summary (forward only) between steps, and steps of two image sizes / token counts through the tape: finite losses, and the
    replayed step after the detour equals the same sequence issued eagerly on a second network bit for bit"""
    from oracle import synth as OS
    blob, over, ocfg, samp = edge_step_inputs()
    blob2 = OS.make_blob(112, 96, 2, 60, seed=29)
    opt = ada_opt(model)
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


# ------------------------------------------------------------------ 5. strict load
@pytest.mark.parametrize('model', MODELS)
def test_state_dict_loads_key_for_key(model):
    """a state_dict() of the restatement loads under caption_model., and the network's state_dict() returns the same keys, shapes and values"""
    from lang2seg_amd import selftest
    opt = ada_opt(model)
    torch.manual_seed(9)
    mod = AdaAttRef(opt)
    net = selftest.build_net(opt, {}, 'f32', None)
    net.load_state_dict({CAP + k: v for k, v in mod.state_dict().items()}, strict=False)
    out = {k: v for k, v in net.state_dict().items() if k.startswith(CAP)}
    want = {CAP + k: v for k, v in mod.state_dict().items()}
    assert list(out) == list(want) and len(want) == 33
    for k, v in want.items():
        assert tuple(out[k].shape) == tuple(v.shape) and torch.equal(out[k], v.detach()), k
