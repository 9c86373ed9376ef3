"""Prediction without ground truth: what the network picks and segments for each sentence of one image, through the device path of
model/eval_device.py (one backbone pass, then per sentence the pick kernel, the n = 1 mask head, the mask kernel and the run-length
encoder).  A zero gt box and a 1 x 1 zero gt mask stand in for the annotations, so the mask kernel's union count is the mask's area."""
import numpy as np
import torch

from .. import ops as O
from . import eval_device as ED


def predict_image(net, data, labels, _pool_words=None):
    """data: {'data': float32 (1, H, W, 3) blob, 'im_info': [H, W, scale]} (+ 'file_name'); labels: int [S][T] token ids, zero padded.
    -> one dict per sentence: file_name, sent_index, category_id, box [x1, y1, x2, y2] (original image), score, area and (networks with a
    mask branch) segmentation {'size': [ih, iw], 'counts': COCO RLE string}."""
    labels = np.asarray(labels)
    if labels.ndim != 2 or labels.shape[0] < 1:
        raise ValueError('labels: an int array [S][T] with S >= 1, got shape %s' % (labels.shape,))
    if ((labels != 0).sum(1) == 0).any():
        raise ValueError('labels: every sentence needs at least one token')
    S = int(labels.shape[0])
    d = dict(data=data['data'], im_info=data['im_info'], labels=labels.astype(np.int64),
             gt_boxes=np.zeros((S, 5), np.float32), gt_masks=np.zeros((S, 1, 1), np.uint8))
    net.eval()
    with_masks = getattr(net, 'variant', None) != 'vgg'         # the VGG16 / Faster R-CNN network has no mask branch
    rec = O.eval_records(S, torch.device(net.device))
    ex = ED._eval_image(net, d, S, rec, 0, with_masks, _pool_words)
    rec_h = rec.cpu()
    if (O.eval_record_fields(rec_h)[0] < 0).any():
        raise ValueError('prediction: no proposal to pick from (empty score matrix)')
    return ex.collect(rec_h, data.get('file_name'), gt=False)
