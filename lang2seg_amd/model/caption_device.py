"""Mask -> sentence: the second half of the cycle for one image.  predict_image's device path (model/predict_device.py) with, behind every
sentence's mask, the caption branch's features under that mask (Network.caption_features) and the captioner's decoding
(Network.caption_decode: greedy, sampled or beam search, nets/decode.py)."""
import numpy as np
import torch

from .. import ops as O
from . import eval_device as ED


def decode_sequence(ix_to_word, seq):
    """lib/misc/utils.py:17-31 for one sentence: the words joined by blanks, up to the first 0 (a word without an entry is a KeyError)"""
    words = []
    for w in seq:
        if int(w) <= 0:
            break
        w = int(w)
        words.append(ix_to_word[str(w)] if str(w) in ix_to_word else ix_to_word[w])     # infos files key by str, Loader.ix_to_word by int
    return ' '.join(words)


def caption_image(net, data, labels, masks=None, sample_max=1, beam_size=1, temperature=1.0, ix_to_word=None, _pool_words=None):
    """predict_image's dicts plus, per sentence, 'caption_tokens', 'caption_logprobs' (and 'caption_beams' for beam search) and 'caption',
    the decoded string, when ix_to_word ({str(id): word}) is given.
    masks: None - the features are pooled under each sentence's PREDICTED mask (the > 122 canvas of the mask kernel, brought to the blob's
    size by the nearest rule of the loader's ground-truth masks) - or uint8 [S][H][W] masks of the blob's size, e.g. the loader's gt_masks.
    The cycle_response network pools the map before and after the gating and uses no mask.
    beam_size > 1 is beam search whatever sample_max says, as in AttModel.sample (:155-156)."""
    from ..nets import decode
    decode.check_args(net, sample_max, beam_size, temperature)
    if getattr(net, 'variant', None) == 'vgg' or not hasattr(net, 'att_embed'):
        raise ValueError('--variant %s has no caption branch on this backbone' % getattr(net, 'variant', '?'))
    labels = np.asarray(labels)
    if labels.ndim != 2 or labels.shape[0] < 1:
        raise ValueError('labels: an int array [S][T] with S >= 1, got shape %s' % (labels.shape,))
    if ((labels != 0).sum(1) == 0).any():
        raise ValueError('labels: every sentence needs at least one token')
    S = int(labels.shape[0])
    H, W = int(np.asarray(data['data']).shape[1]), int(np.asarray(data['data']).shape[2])
    dev = torch.device(net.device)
    if masks is not None:
        masks = torch.as_tensor(np.ascontiguousarray(masks, dtype=np.uint8)) if not isinstance(masks, torch.Tensor) else masks
        if masks.dtype != torch.uint8 or tuple(masks.shape) != (S, H, W):
            raise ValueError('masks: uint8 [S][H][W] at the blob\'s size %s, got %s %s' % ((S, H, W), masks.dtype, tuple(masks.shape)))
        masks = masks.to(dev).contiguous()
    d = dict(data=data['data'], im_info=data['im_info'], labels=labels.astype(np.int64),
             gt_boxes=np.zeros((S, 5), np.float32), gt_masks=np.zeros((S, 1, 1), np.uint8))
    net.eval()
    rec = O.eval_records(S, dev)
    caps = []

    def caption(i, s, ex):
        m = None
        if net.var['cap'] == 'mask':
            if masks is not None:
                m = masks[i]
            else:
                m = net.buf('cap.pred_mask', (H, W), torch.uint8)
                O.mask_resize_nearest(ex.canvas[i], ex.ih, ex.iw, m, H, W)
        att, fc = net.caption_features(m)
        caps.append(net.caption_decode(att, fc, sample_max=sample_max, beam_size=beam_size, temperature=temperature))
    ex = ED._eval_image(net, d, S, rec, 0, True, _pool_words, caption=caption)
    rec_h = rec.cpu()
    if (O.eval_record_fields(rec_h)[0] < 0).any():
        raise ValueError('prediction: no proposal to pick from (empty score matrix)')
    out = ex.collect(rec_h, data.get('file_name'), gt=False)
    for p, c in zip(out, caps):
        p['caption_tokens'], p['caption_logprobs'] = c['seq'], c['logprobs']
        if 'beams' in c:
            p['caption_beams'] = [dict(seq=b['seq'], logps=b['logps'], p=b['p']) for b in c['beams']]
        if ix_to_word is not None:
            p['caption'] = decode_sequence(ix_to_word, c['seq'])
    return out
