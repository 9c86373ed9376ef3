"""The general expression encoder on the device: GRU / tanh-RNN step kernels, stacked layers, one direction (csrc/rnn_step.hip and
nets/resnet_v1.py _encoder_fwd / _encoder_bwd) against torch.nn.LSTM / GRU / RNN on the CPU in float32.
Bounds: those of tests/test_kernels_gpu.py for this family (its rel_err): 1e-5 forward, 1e-4 gradients."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from rnn_encoder_util import (CONFIGS, PRE, GATES, rel_err, torch_rnn, enc_opt, rnn_state, make_sd, LayeredRNN, run_module, GeneralOracleNet,
                              edge_step_inputs, torch_encoder)

pytestmark = pytest.mark.gpu

DEV = 'cuda'
FWD_TOL, GRAD_TOL = 1e-5, 1e-4
NAMES = ['rpn_cross_entropy', 'rpn_loss_box', 'cross_entropy', 'loss_box', 'loss_mask', 'loss_caption', 'total_loss']


def ops():
    from lang2seg_amd import ops as O
    return O


# ------------------------------------------------------------------ 1. the step entries alone
def _run_steps(O, typ, mod, x, dhid, T, H, ndir):
    """one layer through l2s_linear_fwd + the step entries, forward and backward; returns per-step h [T][ndir H] and the gradients"""
    G, I = GATES[typ], x.shape[1]
    sd = {k: v.detach().to(DEV).contiguous() for k, v in mod.state_dict().items()}
    xd = x.to(DEV)
    z = lambda *s: torch.zeros(*s, device=DEV)
    st = []
    for sfx in ['', '_reverse'][:ndir]:
        q = dict(sfx=sfx, g=z(T, G * H), hs=z(T + 1, H), act=z(T, 4 * H), dgi=z(T, G * H), dgh=z(T, G * H), carry=z(2, H),
                 wT=sd['weight_hh_l0' + sfx].t().contiguous())
        O.linear_fwd(xd, sd['weight_ih_l0' + sfx], sd['bias_ih_l0' + sfx], q['g'], T, G * H, I)
        st.append(q)
    fwd, bwd = (O.gru_step_fwd, O.gru_step_bwd) if typ == 'gru' else (O.rnn_step_fwd, O.rnn_step_bwd)
    for s_ in range(T):
        dirs = []
        for di, q in enumerate(st):
            tt = s_ if di == 0 else T - 1 - s_
            cur, prev = (tt + 1, tt) if di == 0 else (tt, tt + 1)
            dirs.append(dict(w_hh=sd['weight_hh_l0' + q['sfx']], b_hh=sd['bias_hh_l0' + q['sfx']], gates_in=q['g'][tt], h_prev=q['hs'][prev],
                             h=q['hs'][cur], act=q['act'][tt]))
        fwd(dirs, H)
    dh = dhid.to(DEV)
    k = 0
    for s_ in range(T):
        dirs = []
        for di, q in enumerate(st):
            tt = T - 1 - s_ if di == 0 else s_
            nxt = tt + 1 if di == 0 else tt - 1
            cur, prev = (tt + 1, tt) if di == 0 else (tt, tt + 1)
            ext = dh[di * H:(di + 1) * H] if s_ == 0 else None
            if typ == 'gru':
                dirs.append(dict(w_hh_T=q['wT'], dgh_next=(q['dgh'][nxt] if s_ > 0 else None), dh_ext=ext, dh_carry_in=(q['carry'][k] if s_ > 0 else None),
                                 act=q['act'][tt], h_prev=q['hs'][prev], dgi=q['dgi'][tt], dgh=q['dgh'][tt], dh_carry_out=q['carry'][1 - k]))
            else:
                dirs.append(dict(w_hh_T=q['wT'], dg_next=(q['dgi'][nxt] if s_ > 0 else None), dh_ext=ext, h=q['hs'][cur], dg=q['dgi'][tt]))
        bwd(dirs, H)
        k = 1 - k
    out = {}
    dx = z(T, I)
    for di, q in enumerate(st):
        sfx = q['sfx']
        dgh = q['dgh'] if typ == 'gru' else q['dgi']
        hprev = q['hs'][0:T] if di == 0 else q['hs'][1:T + 1]
        dwh, dbh, dwi, dbi = z(G * H, H), z(G * H), z(G * H, I), z(G * H)
        O.linear_bwd_w(dgh, hprev, dwh, dbh, T, G * H, H)
        O.linear_bwd_w(q['dgi'], xd, dwi, dbi, T, G * H, I)
        O.linear_bwd_x(q['dgi'], sd['weight_ih_l0' + sfx], dx, T, G * H, I, accumulate=True)
        out.update({'weight_hh_l0' + sfx: dwh, 'bias_hh_l0' + sfx: dbh, 'weight_ih_l0' + sfx: dwi, 'bias_ih_l0' + sfx: dbi})
    torch.cuda.synchronize()
    h = torch.cat([st[0]['hs'][1:T + 1]] + [q['hs'][0:T] for q in st[1:]], dim=1)
    return h, out, dx


@pytest.mark.parametrize('ndir', [1, 2])
@pytest.mark.parametrize('H,T', [(8, 1), (260, 3), (512, 5)])
@pytest.mark.parametrize('typ', ['gru', 'rnn'])
def test_step_kernels_vs_torch(typ, H, T, ndir):
    """H = 8: one partial workgroup, two live lanes per wave; H = 260: 65 workgroups, a ragged second trip of the float4 loop; H = 512: the
    product's size.  h of every step and the W_ih / W_hh / b_ih / b_hh / x gradients for a random d(hidden) against torch autograd."""
    O = ops()
    I = 128
    mod = torch_rnn(typ, I, H, 1, ndir == 2, seed=H + T)
    g = torch.Generator().manual_seed(7 * H + T + ndir)
    x = torch.randn(T, I, generator=g)
    dhid = torch.randn(ndir * H, generator=g)
    xr = x.clone().requires_grad_(True)
    out_ref, hn = mod(xr.unsqueeze(1))
    (hn.reshape(-1) * dhid).sum().backward()
    h, grads, dx = _run_steps(O, typ, mod, x, dhid, T, H, ndir)
    e = rel_err(h, out_ref.squeeze(1))
    print('step %s H=%d T=%d ndir=%d: h %.2e' % (typ, H, T, ndir, e), end='')
    errs = {k: rel_err(grads[k], p.grad) for k, p in mod.named_parameters()}
    errs['x'] = rel_err(dx, xr.grad)
    print('  grads ' + ' '.join('%s %.2e' % kv for kv in errs.items()))
    assert e < FWD_TOL
    for k, v in errs.items():
        assert v < GRAD_TOL, (k, v)


@pytest.mark.parametrize('typ', ['gru', 'rnn'])
def test_step_entries_reject_bad_shapes_before_any_launch(typ):
    from lang2seg_amd._lib import L2SError
    O = ops()
    fwd, bwd = (O.gru_step_fwd, O.gru_step_bwd) if typ == 'gru' else (O.rnn_step_fwd, O.rnn_step_bwd)
    H = 6
    buf = torch.full((64 * H,), 7.0, device=DEV)
    d = {k: buf for k in ('w_hh', 'b_hh', 'gates_in', 'h_prev', 'h', 'act', 'w_hh_T', 'dgh_next', 'dg_next', 'dh_ext', 'dh_carry_in', 'dgi', 'dgh',
                          'dg', 'dh_carry_out')}
    for fn in (fwd, bwd):
        with pytest.raises(L2SError):
            fn([d], H)                      # H % 4 != 0
        with pytest.raises(L2SError):
            fn([d, d, d], 8)                # ndir = 3
    torch.cuda.synchronize()
    assert bool((buf == 7.0).all())         # nothing was launched


# ------------------------------------------------------------------ 2. the network's own encoder
_NETS = {}


def _enc_net(typ, layers, bidir, H=64):
    """one small-encoder network per configuration (ResNet-50 trunk: the encoder does not see it)"""
    key = (typ, layers, bidir, H)
    if key not in _NETS:
        from lang2seg_amd import selftest
        opt = enc_opt(typ, layers, bidir, H=H, vocab_size=60)
        sd = make_sd(opt, seed=3)
        sd = {k: v for k, v in sd.items() if k.startswith(('rnn_encoder.', 'dynamic_fc', 'response_fc'))}
        net = selftest.build_net(opt, {}, 'f32', None, num_layers=50)
        net.load_state_dict(sd)
        _NETS[key] = (net, opt, sd)
    return _NETS[key]


@pytest.mark.parametrize('typ,layers,bidir', CONFIGS)
def test_encoder_vs_torch(typ, layers, bidir):
    """hidden (order included) and every encoder parameter gradient through Network._encoder_fwd / _encoder_bwd, T in {1, 4}, without
    dropout and with an injected inter-layer mask (the same mask between separately run torch layers).  Printed beside each error: the
    device's and the CPU float32 torch's own error against a float64 torch run (a record, not a gate)."""
    net, opt, sd = _enc_net(typ, layers, bidir)
    H, ndir = opt['rnn_hidden_size'], 2 if bidir else 1
    net.train()
    g = torch.Generator().manual_seed(31)
    for T in (1, 4):
        for with_mask in ([False, True] if layers > 1 else [False]):
            labels = torch.randint(1, 60, (T,), generator=g)
            dhid = torch.randn(layers * ndir * H, generator=g)
            masks = [(torch.rand(T, ndir * H, generator=g) > 0.2).float() / 0.8 for _ in range(layers - 1)] if with_mask else None
            net.parity = dict(drops={'rnn_l%d' % l: masks[l].to(DEV) for l in range(layers - 1)} if with_mask else {})
            net.t = {}
            d = dict(T=T, labels=labels.to(DEV))
            hidden = net._encoder_fwd(d)
            net.P.grad.zero_()
            net._encoder_bwd(d, dhid.to(DEV))
            torch.cuda.synchronize()
            h32, g32 = torch_encoder(sd, opt, labels, masks, dhid, torch.float32)
            h64, g64 = torch_encoder(sd, opt, labels, masks, dhid, torch.float64)
            tag = '%s x%d %s T=%d%s' % (typ, layers, 'bi' if bidir else 'uni', T, ' mask' if with_mask else '')
            rows = [('hidden', hidden, h32, h64, FWD_TOL)]
            for k in g32:
                rows.append((k, net.P.view(k, net.P.grad).view(net.P.shapes[k]), g32[k], g64[k], GRAD_TOL))
            worst, bad = {}, []
            for k, dev_, r32, r64, tol in rows:
                e = rel_err(dev_, r32)
                w = worst.setdefault('hidden' if k == 'hidden' else 'grad', [0.0, 0.0, 0.0])
                w[0], w[1], w[2] = max(w[0], e), max(w[1], rel_err(dev_, r64)), max(w[2], rel_err(r32, r64))
                if not e < tol:
                    bad.append((k, e))
            for kind, w in worst.items():
                print('encoder %-22s %-6s vs torch f32 %.2e | device vs f64 %.2e | torch f32 vs f64 %.2e' % (tag, kind, w[0], w[1], w[2]))
            assert not bad, (tag, bad)
    net.parity = None


# ------------------------------------------------------------------ 3. the whole step against the oracle
@pytest.mark.parametrize('variant,typ,layers,bidir', [('cycle', 'gru', 2, 1), ('cycle', 'rnn', 1, 0), ('vgg', 'gru', 1, 1)])
def test_whole_step_vs_oracle(variant, typ, layers, bidir):
    """the recipe of test_edge_cases_vs_oracle (96x128 blob, vocab 60, recorded sampling keys, the device's proposals forced into the
    oracle): losses within 1e-3, integer targets exact, all gradients finite, the encoder weights after one SGD step within 1e-4."""
    from lang2seg_amd import selftest
    from lang2seg_amd.model.train_val import make_optimizer
    from oracle import weights as OW
    blob, over, ocfg, samp = edge_step_inputs()
    opt = enc_opt(typ, layers, bidir)
    if variant == 'vgg':
        opt['C4_feat_dim'] = 512
    sd = make_sd(opt, seed=3, variant=variant)
    net = selftest.build_net(opt, over, 'f32', sd, variant=variant)
    net.parity = selftest.parity_from_samp(samp)
    lv = net.forward_backward(net.upload_blob(blob, 0)).cpu().numpy()
    n = int(net.t['proposal_n'].item())
    assert n > 0
    samp['forced_proposals'] = (net.t['proposal_rois'].cpu().numpy()[:n], net.t['proposal_scores'].cpu().numpy()[:n])
    onet = GeneralOracleNet(sd, opt, ocfg, variant=variant)
    T, L = onet.forward_train(blob, samp)
    slots = net._loss_slots()
    for i, k in zip(slots, OW.loss_keys(variant)):
        ref = float(L[k])
        assert np.isfinite(lv[i]) and abs(lv[i] - ref) < 1e-3 * max(1.0, abs(ref)), (variant, typ, k, lv[i], ref)
    assert rel_err(net.t['hidden'], T['hidden'].reshape(-1)) < FWD_TOL
    assert np.array_equal(net.t['labels'].cpu().numpy().astype(np.int64), np.asarray(T['labels']).reshape(-1).astype(np.int64))
    assert np.array_equal(net.t['rpn_labels'].cpu().numpy().astype(np.int64), np.asarray(T['rpn_labels']).reshape(-1).astype(np.int64))
    assert bool(torch.isfinite(net.P.grad).all())
    enc = [k for k in net.P.trainable if k.startswith('rnn_encoder.')]
    assert all(float(net.P.view(k, net.P.grad).abs().max()) > 0 for k in enc if k != 'rnn_encoder.embedding.weight')
    onet.backward()
    sgd = make_optimizer(net)
    sgd.step()
    onet.sgd_step(lr=sgd.lr)
    torch.cuda.synchronize()
    sd1 = net.state_dict()
    for k in enc:
        e = rel_err(sd1[k], onet.p[k].detach())
        print('step %s %s x%d: %s after SGD %.2e' % (variant, typ, layers, k, e))
        assert e < GRAD_TOL, (k, e)
        assert not np.array_equal(sd1[k].numpy(), sd[k]) or k == 'rnn_encoder.embedding.weight'          # it did move


# ------------------------------------------------------------------ 4. launch tape and determinism
def _tape_net(opt, sd, over, tape):
    from lang2seg_amd import selftest
    from lang2seg_amd.optim import SGD
    net = selftest.build_net(opt, over, 'f32', sd)
    net.use_tape = tape
    return net, SGD(net, 0.0, keep_grad=True)          # lr 0: the weights stay put, the steps differ by their dropout masks and sampling keys


def test_tape_replay_and_determinism_gru2():
    """(gru, 2 layers, bidirectional), three whole steps with the production RNG (word and inter-layer dropout on, sampling keys from the
    device counter): replayed from the launch tape they equal the eagerly issued steps bit for bit - `hidden` and the whole gradient
    buffer after every step - and a second eager run gives the same bits again.  Only the reported loss scalars, which the loss kernels
    add up with float atomics and no gradient reads, are compared with a tolerance.  Then the encoder alone on a tape of its own, with
    a fixed d(hidden) and new tokens per replay."""
    from lang2seg_amd import ops as O
    blob, over, ocfg, samp = edge_step_inputs()
    opt = enc_opt('gru', 2, 1)
    sd = make_sd(opt, seed=3)
    res = []
    for tape in (False, True, False):
        net, sgd = _tape_net(opt, sd, over, tape)
        steps = []
        for _ in range(3):
            lv = net.train_step(dict(blob), 0, sgd)
            torch.cuda.synchronize()
            steps.append((np.asarray(lv), net.t['hidden'].clone(), net.P.grad.clone()))
        if tape:
            assert len(net._tapes) == 1
        res.append(steps)
    enc_lo = min(net.P.offsets[k] for k in net.P.trainable if k.startswith('rnn_encoder.'))
    enc_hi = max(net.P.offsets[k] + int(np.prod(net.P.shapes[k])) for k in net.P.trainable if k.startswith('rnn_encoder.'))
    for s_, (a, b, c) in enumerate(zip(*res)):
        assert torch.equal(a[1], b[1]) and torch.equal(a[1], c[1]), s_                     # hidden: replay == eager == eager again
        assert float(a[2][enc_lo:enc_hi].abs().max()) > 0
        assert torch.equal(a[2], b[2]), ('tape vs eager', s_, int((a[2] != b[2]).sum()))   # every gradient of the step, bit for bit
        assert torch.equal(a[2], c[2]), ('run vs run', s_, int((a[2] != c[2]).sum()))
        assert np.allclose(a[0], b[0], rtol=1e-5, atol=1e-6) and np.allclose(a[0], c[0], rtol=1e-5, atol=1e-6), (s_, a[0], b[0], c[0])
    assert not torch.equal(res[0][0][1], res[0][1][1])                                      # the dropout masks did change between steps
    assert not torch.equal(res[0][0][2][enc_lo:enc_hi], res[0][1][2][enc_lo:enc_hi])
    # the encoder alone on a tape of its own: fixed d(hidden), three replays with new tokens
    net = _tape_net(opt, sd, over, False)[0]
    net.train(); net.parity = None
    main = torch.cuda.current_stream()
    T = 4
    g = torch.Generator().manual_seed(5)
    lab = torch.randint(1, 60, (T,), generator=g).to(DEV)
    dhid = torch.randn(4 * 512, generator=g).to(DEV)
    d = dict(T=T, labels=lab)
    enc = [k for k in net.P.trainable if k.startswith('rnn_encoder.')]
    grads = lambda: torch.cat([net.P.view(k, net.P.grad) for k in enc]).clone()

    def issue():
        for k in enc:
            O.memset_zero(net.P.view(k, net.P.grad))
        hid = net._encoder_fwd(d)
        net._encoder_bwd(d, dhid)
        return hid
    net.t = {}
    issue()                             # the activation plan exists now: a buffer's clear is a launch (a first use clears by allocation)
    torch.cuda.synchronize()
    h = O.tape_begin([main])
    try:
        hid = issue()
    finally:
        O.tape_end(h)
    torch.cuda.synchronize()
    n_launch = O.tape_size(h)
    assert n_launch > 0
    for rep in range(3):
        lab.copy_(torch.randint(1, 60, (T,), generator=g)); dhid.copy_(torch.randn(4 * 512, generator=g))
        # (the recorded dropout launches draw from the device step counter: hold it still so that replay and eager see the same masks)
        c0 = net.seed_counter().clone()
        O.tape_run(h, [main]); torch.cuda.synchronize()
        a = (hid.clone(), grads())
        net.seed_counter().copy_(c0)
        issue(); torch.cuda.synchronize()
        b = (hid.clone(), grads())
        net.seed_counter().copy_(c0)
        issue(); torch.cuda.synchronize()
        c = (hid.clone(), grads())
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), rep                    # replayed == eager, bit for bit
        assert torch.equal(b[0], c[0]) and torch.equal(b[1], c[1]), rep                    # two runs: identical gradient bits
        assert float(a[1].abs().max()) > 0


# ------------------------------------------------------------------ 5. TEST mode
def test_test_mode_gru2_unidirectional():
    """(gru, 2 layers, one direction): predict_image on a synthetic image returns one dict per sentence, and forward_test_sentence's
    `hidden` is the torch module's (eval mode: no inter-layer dropout)"""
    from lang2seg_amd import selftest
    from lang2seg_amd.loaders.synthetic_loader import SyntheticLoader
    from lang2seg_amd.model.predict_device import predict_image
    opt = enc_opt('gru', 2, 0)
    sd = make_sd(opt, seed=3)
    net = selftest.build_net(opt, {}, 'f32', sd)
    b = SyntheticLoader(num_images=1, sents_per_image=3, H=224, W=288, T=6, vocab_size=60, seed=0)._image(0)
    data = dict(data=b['data'], im_info=b['im_info'], file_name=b['file_name'])
    out = predict_image(net, data, np.asarray(b['labels']))
    assert len(out) == 3 and [p['sent_index'] for p in out] == [0, 1, 2]
    assert all(len(p['box']) == 4 and 0.0 < p['score'] <= 1.0 and 'segmentation' in p for p in out)
    net.eval()
    blob = dict(b); blob['gt_boxes'] = np.zeros((3, 5), np.float32); blob['gt_masks'] = np.zeros((3, 1, 1), np.uint8)
    dev = net.upload_blob(blob, 1)
    net.forward_test_image(dev)
    net.forward_test_sentence(dev)
    torch.cuda.synchronize()
    mod = torch_rnn('gru', 512, 512, 2, 0)
    mod.load_state_dict({k[len(PRE):]: torch.from_numpy(v) for k, v in sd.items() if k.startswith(PRE)})
    lab = dev['labels'].cpu()
    with torch.no_grad():
        x = F.relu(F.linear(torch.from_numpy(sd['rnn_encoder.embedding.weight'])[lab], torch.from_numpy(sd['rnn_encoder.mlp.0.weight']),
                            torch.from_numpy(sd['rnn_encoder.mlp.0.bias'])))
        ref = run_module(mod, x)
    assert net.t['hidden'].numel() == 2 * 512
    assert rel_err(net.t['hidden'], ref) < FWD_TOL


# ------------------------------------------------------------------ 6. checkpoints
def test_snapshot_roundtrip_and_mismatch_gru2(tmp_path):
    """SolverWrapper.snapshot of a (gru, 2, bidirectional) network after one real update, restored by from_snapshot into a fresh network:
    every tensor is the same bits, and so is the next step - `hidden` and the whole gradient buffer (the reported loss scalars, summed by
    the loss kernels with float atomics that no gradient reads, within 1e-5); loading the file into a default (lstm) network is an
    error that names rnn_type"""
    from lang2seg_amd import selftest
    from lang2seg_amd.loaders.synthetic_loader import SyntheticLoader
    from lang2seg_amd.model.train_val import SolverWrapper
    from lang2seg_amd.optim import SGD
    blob, over, ocfg, samp = edge_step_inputs()
    opt = enc_opt('gru', 2, 1)
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
    assert any(not np.array_equal(sa[k].numpy(), sd[k]) for k in sa if k.startswith(PRE))
    b.parity = selftest.parity_from_samp(samp)
    b.train()
    la = a.forward_backward(a.upload_blob(blob, 0)).cpu().numpy()
    lb = b.forward_backward(b.upload_blob(blob, 0)).cpu().numpy()
    torch.cuda.synchronize()
    assert torch.equal(a.t['hidden'], b.t['hidden'])
    assert float(a.P.grad.abs().max()) > 0
    assert torch.equal(a.P.grad, b.P.grad), int((a.P.grad != b.P.grad).sum())
    assert np.allclose(la, lb, rtol=1e-5, atol=1e-6), (la, lb)
    lstm = selftest.build_net(enc_opt('lstm', 1, 1), over, 'f32', None)
    with pytest.raises(ValueError, match='rnn_type'):
        SolverWrapper(lstm, ld, str(tmp_path / 'out'), str(tmp_path / 'tb')).from_snapshot(sfile, nfile)
    with pytest.raises(ValueError, match='rnn_type'):
        lstm.load_state_dict(torch.load(sfile, map_location='cpu'))
