"""Shared by tests/test_rnn_encoder_{cpu,gpu}.py: the oracle of the general expression encoder is torch.nn.LSTM / GRU / RNN on the CPU -
the very op the reference calls (lang_encoder.py:21-24) - with its state dict copied key for key under 'rnn_encoder.rnn.'."""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import net as ON
from oracle import weights as OW

PRE = 'rnn_encoder.rnn.'
GATES = {'lstm': 4, 'gru': 3, 'rnn': 1}
sig = torch.sigmoid
# (rnn_type, rnn_num_layers, bidirectional)
CONFIGS = [('gru', 1, 1), ('gru', 2, 1), ('gru', 2, 0), ('rnn', 1, 1), ('lstm', 2, 1), ('lstm', 1, 0), ('lstm', 3, 0)]


def rel_err(a, b):
    """tests/test_kernels_gpu.py's: max |a - b| over the reference's max magnitude"""
    a = torch.as_tensor(a).detach().double().cpu(); b = torch.as_tensor(b).detach().double().cpu()
    return float((a - b).abs().max() / (b.abs().max() + 1e-12))


def torch_rnn(typ, in_size, H, layers, bidir, seed=0, dtype=torch.float32):
    torch.manual_seed(seed)
    m = getattr(torch.nn, typ.upper())(in_size, H, layers, bidirectional=bool(bidir))
    return m.to(dtype)


def enc_opt(typ, layers, bidir, H=512, **kw):
    opt = OW.default_opt(vocab_size=kw.pop('vocab_size', 60), seq_length=kw.pop('seq_length', 6))
    opt.update(rnn_type=typ, rnn_num_layers=layers, bidirectional=bidir, rnn_hidden_size=H)
    opt.update(kw)
    return opt


def rnn_state(mod):
    return {PRE + k: v.detach().float().numpy().copy() for k, v in mod.state_dict().items()}


def make_sd(opt, seed=3, variant='cycle', head_gain=4.0, rnn_seed=11):
    """oracle.weights.make_state_dict's dict with its (single bi-LSTM layer) encoder entries replaced by a seeded torch module's"""
    sd = OW.make_state_dict(opt, seed=seed, head_gain=head_gain, variant=variant)
    for k in [k for k in sd if k.startswith(PRE)]:
        del sd[k]
    sd.update(rnn_state(torch_rnn(opt['rnn_type'], opt['word_vec_size'], opt['rnn_hidden_size'], opt['rnn_num_layers'], opt['bidirectional'], rnn_seed)))
    return sd


class LayeredRNN(object):
    """a stacked torch.nn.LSTM / GRU / RNN run as separate one-layer modules, so that a given mask can be applied between the layers
    (what the module's own `dropout` does with a mask it draws itself).  Parameters: {torch key: leaf tensor}; `hidden` is h_n
    flattened as lang_encoder.py:76-80 does for batch 1: index (layer * ndir + dir) * H."""

    def __init__(self, typ, params, layers, bidir, dtype=torch.float32):
        self.typ, self.layers, self.ndir = typ, layers, 2 if bidir else 1
        self.p = {k: torch.as_tensor(v).detach().clone().to(dtype).requires_grad_(True) for k, v in params.items()}
        self.dtype = dtype

    def _layer(self, l, x):
        """layer l as a one-layer torch module called on this object's leaf tensors"""
        from torch.func import functional_call
        sfxs = ['', '_reverse'][:self.ndir]
        p = {n + '_l0' + sfx: self.p[n + '_l%d%s' % (l, sfx)] for sfx in sfxs for n in ('weight_ih', 'weight_hh', 'bias_ih', 'bias_hh')}
        H, K = p['weight_hh_l0'].shape[1], p['weight_ih_l0'].shape[1]
        mod = getattr(torch.nn, self.typ.upper())(K, H, 1, bidirectional=self.ndir == 2).to(self.dtype)
        out = functional_call(mod, p, (x.unsqueeze(1),))
        hn = out[1][0] if isinstance(out[1], tuple) else out[1]
        return out[0].squeeze(1), hn.reshape(-1)

    def forward(self, x, masks=None):
        hs = []
        for l in range(self.layers):
            x, hn = self._layer(l, x)
            hs.append(hn)
            if masks is not None and l + 1 < self.layers and masks[l] is not None:
                x = x * masks[l].to(self.dtype)
        return torch.cat(hs)


def run_module(mod, x):
    """the module itself: hidden flattened as ENC:76-80"""
    out = mod(x.unsqueeze(1))
    hn = out[1][0] if isinstance(out[1], tuple) else out[1]
    return hn.reshape(-1)


class GeneralOracleNet(ON.OracleNet):
    """oracle.net.OracleNet with rnn_encoder in the reference's general form: getattr(nn, rnn_type.upper())(word_vec_size, hidden_size,
    n_layers, bidirectional=...) on the same leaf tensors the rest of the oracle differentiates"""

    def rnn_encoder(self, labels, word_drop=None, masks=None):
        emb = self.p['rnn_encoder.embedding.weight'][labels[0]]
        if word_drop is not None:
            emb = emb * word_drop
        x = F.relu(F.linear(emb, self.p['rnn_encoder.mlp.0.weight'], self.p['rnn_encoder.mlp.0.bias']))
        o = self.opt
        enc = LayeredRNN.__new__(LayeredRNN)
        enc.typ, enc.layers, enc.ndir, enc.dtype = o['rnn_type'], o['rnn_num_layers'], 2 if o['bidirectional'] else 1, torch.float32
        enc.p = {k[len(PRE):]: v for k, v in self.p.items() if k.startswith(PRE)}
        return enc.forward(x, masks).unsqueeze(0)


def torch_encoder(sd, opt, labels, masks, dhid, dtype):
    """embedding -> mlp (ReLU) -> the stacked torch cell, in `dtype`; returns hidden and {key: gradient}"""
    p = {k: torch.from_numpy(np.asarray(v)).to(dtype).requires_grad_(True) for k, v in sd.items() if k.startswith('rnn_encoder.') and not k.startswith(PRE)}
    lay = LayeredRNN(opt['rnn_type'], {k[len(PRE):]: v for k, v in sd.items() if k.startswith(PRE)}, opt['rnn_num_layers'], opt['bidirectional'], dtype)
    x = F.relu(F.linear(p['rnn_encoder.embedding.weight'][labels], p['rnn_encoder.mlp.0.weight'], p['rnn_encoder.mlp.0.bias']))
    hid = lay.forward(x, masks)
    (hid * dhid.to(dtype)).sum().backward()
    grads = {k: v.grad for k, v in p.items()}
    grads.update({PRE + k: v.grad for k, v in lay.p.items()})
    return hid.detach(), grads


class TorchOps(object):
    """the entry points the encoder calls (lang2seg_amd.ops), restated with torch on whatever device the tensors live on: lets the CPU tests
    run Network._encoder_fwd / _encoder_bwd - the host's order of launches, buffers, slices and keys - without a GPU.  The kernels
    themselves are checked on the device (tests/test_rnn_encoder_gpu.py).  Only the argument forms the encoder uses are restated; every
    other one is asserted to be at its default, so a call this class does not model fails instead of passing silently."""
    @staticmethod
    def linear_fwd(x, w, b, y, M, N, K, act=0, accumulate=False, ldx=None, ldy=None, ldw=None):
        assert ldx is None and ldy is None and ldw is None and act in (0, 1, 2)      # dense rows only: what the encoder passes
        r = x.view(-1)[:M*K].view(M, K) @ w.view(-1)[:N*K].view(N, K).t() + (b.view(-1)[:N] if b is not None else 0)
        yv = y.view(-1)[:M*N].view(M, N)
        if accumulate: r = r + yv
        yv.copy_(F.relu(r) if act == 1 else torch.tanh(r) if act == 2 else r)
    @staticmethod
    def linear_bwd_x(dy, w, dx, M, N, K, accumulate=False, lddy=None, lddx=None, mul=None, ws=None):
        assert lddy is None and lddx is None and mul is None
        r = dy.view(-1)[:M*N].view(M, N) @ w.view(-1)[:N*K].view(N, K)
        dv = dx.view(-1)[:M*K].view(M, K)
        dv.copy_(dv + r if accumulate else r)
    @staticmethod
    def linear_bwd_x_ws_floats(M, N, K): return 0
    @staticmethod
    def linear_bwd_w(dy, x, dw, db, M, N, K, lddy=None, ldx=None):
        assert lddy is None and ldx is None
        dyv = dy.reshape(-1)[:M*N].view(M, N); xv = x.reshape(-1)[:M*K].view(M, K)
        dw.view(N, K).add_(dyv.t() @ xv); db.view(N).add_(dyv.sum(0))
    @staticmethod
    def act_bwd(dy, y, act):
        assert act == 1
        dy.mul_((y > 0).float())
    @staticmethod
    def embed_fwd(table, ids, mask, out, T, D, relu):
        assert not relu
        out.copy_(table.view(-1, D)[ids] * (mask if mask is not None else 1))
    @staticmethod
    def embed_bwd(dout, out, ids, mask, dtable, T, D, relu):
        assert not relu
        dtable.view(-1, D).index_add_(0, ids, dout * (mask if mask is not None else 1))
    @staticmethod
    def memcpy(dst, src): dst.copy_(src)
    @staticmethod
    def memset_zero(t): t.zero_()
    @staticmethod
    def lstm_step_fwd(dirs, H):
        for d in dirs:
            g = d['gates_in'] + d['w_hh'].view(4*H, H) @ d['h_prev'] + d['b_hh']
            i, f, gg, o = sig(g[:H]), sig(g[H:2*H]), torch.tanh(g[2*H:3*H]), sig(g[3*H:])
            c = f * d['c_prev'] + i * gg
            d['c'].copy_(c); d['h'].copy_(o * torch.tanh(c)); d['act'].copy_(torch.cat([i, f, gg, o])); d['gates_out'].copy_(g)
    @staticmethod
    def lstm_step_bwd(dirs, H):
        for d in dirs:
            dh = torch.zeros(H)
            if d.get('dgates_next') is not None: dh = d['w_hh_T'].view(H, 4*H) @ d['dgates_next']
            if d.get('dh_ext') is not None: dh = dh + d['dh_ext']
            a = d['act']; i, f, gg, o = a[:H], a[H:2*H], a[2*H:3*H], a[3*H:]
            tc = torch.tanh(d['c']); dcn = d['dc_in'] + dh * o * (1 - tc*tc)
            d['dgates'].copy_(torch.cat([dcn*gg*i*(1-i), dcn*d['c_prev']*f*(1-f), dcn*i*(1-gg*gg), dh*tc*o*(1-o)])); d['dc_prev'].copy_(dcn*f)
    @staticmethod
    def gru_step_fwd(dirs, H):
        for d in dirs:
            a = d['w_hh'].view(3*H, H) @ d['h_prev'] + d['b_hh']; gi = d['gates_in']
            r, z = sig(gi[:H] + a[:H]), sig(gi[H:2*H] + a[H:2*H]); n = torch.tanh(gi[2*H:] + r * a[2*H:])
            d['h'].copy_((1-z)*n + z*d['h_prev']); d['act'].copy_(torch.cat([r, z, n, a[2*H:]]))
    @staticmethod
    def gru_step_bwd(dirs, H):
        for d in dirs:
            dh = torch.zeros(H)
            if d.get('dgh_next') is not None: dh = d['w_hh_T'].view(H, 3*H) @ d['dgh_next']
            if d.get('dh_ext') is not None: dh = dh + d['dh_ext']
            if d.get('dh_carry_in') is not None: dh = dh + d['dh_carry_in']
            a = d['act']; r, z, n, an = a[:H], a[H:2*H], a[2*H:3*H], a[3*H:]
            dn = dh*(1-z); dz = dh*(d['h_prev']-n); dan = dn*(1-n*n); daz = dz*z*(1-z); dar = dan*an*r*(1-r)
            d['dgi'].copy_(torch.cat([dar, daz, dan])); d['dgh'].copy_(torch.cat([dar, daz, dan*r])); d['dh_carry_out'].copy_(dh*z)
    @staticmethod
    def rnn_step_fwd(dirs, H):
        for d in dirs: d['h'].copy_(torch.tanh(d['gates_in'] + d['w_hh'].view(H, H) @ d['h_prev'] + d['b_hh']))
    @staticmethod
    def rnn_step_bwd(dirs, H):
        for d in dirs:
            dh = torch.zeros(H)
            if d.get('dg_next') is not None: dh = d['w_hh_T'].view(H, H) @ d['dg_next']
            if d.get('dh_ext') is not None: dh = dh + d['dh_ext']
            d['dg'].copy_(dh * (1 - d['h']*d['h']))
    @staticmethod
    def rnn_concat_fwd(hs, mask, out, T, H):
        r = torch.cat([h[:T] for h in hs], 1); out.copy_(r * mask if mask is not None else r)
    @staticmethod
    def rnn_concat_bwd(dx, mask, adds, ds, T, H):
        v = dx * mask if mask is not None else dx.clone()
        for i, dd in enumerate(ds):
            dd.copy_(v[:, i*H:(i+1)*H])
            if adds[i] is not None: dd[T-1 if i == 0 else 0] += adds[i]
    NAMES = ('linear_fwd', 'linear_bwd_x', 'linear_bwd_x_ws_floats', 'linear_bwd_w', 'act_bwd', 'embed_fwd', 'embed_bwd', 'memcpy', 'memset_zero',
             'lstm_step_fwd', 'lstm_step_bwd', 'gru_step_fwd', 'gru_step_bwd', 'rnn_step_fwd', 'rnn_step_bwd', 'rnn_concat_fwd', 'rnn_concat_bwd')


def edge_step_inputs(H=96, W=128, T=4, seed=23):
    """the recipe of tests/test_train_step_gpu.py::test_edge_cases_vs_oracle ('small_image'): blob, config overrides, recorded sampling keys"""
    import copy
    from oracle import synth as OS
    blob = OS.make_blob(H, W, T, 60, seed=seed)
    over = dict(BATCH_SIZE=16, RPN_PRE_NMS_TOP_N=600, RPN_POST_NMS_TOP_N=100, RPN_BATCHSIZE=64)
    ocfg = copy.deepcopy(ON.DEFAULT_CFG); ocfg['TRAIN'].update(over)
    nA = -(-H // 16) * -(-W // 16) * 12
    rs = np.random.RandomState(1)
    samp = dict(rpn_fg_keys=rs.permutation(nA).astype(np.uint32), rpn_bg_keys=rs.permutation(nA).astype(np.uint32),
                roi_fg_keys=rs.permutation(100).astype(np.uint32), roi_bg_keys=rs.permutation(100).astype(np.uint32))
    return blob, over, ocfg, samp
