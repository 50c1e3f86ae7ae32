"""Drop-in counterpart of the reference's ``model/grad_nets.py``: ``model/nets.py`` with one change —
both functions also return ``grad_in``, the conv5_3 output before the channel L2 norm
(model/grad_nets.py:63, :129), so that a gradient can be taken at that map and shown on the image.

The network lives in ``model/nets.py``; both functions are ``VGG16NetVLAD.forward_with_map``, the
code path of ``nets.vgg16Netvlad`` / ``nets.vgg16`` themselves, so the first return values are theirs
bit for bit (the forced ``prepack`` and the plane images of the assignment weights included).
``grad_in`` is ``VGG16NetVLAD.features()``' tensor in the model's compute dtype (float32 or bf16) and
the very node the first value was computed from: ``torch.autograd.grad(f(first), grad_in)`` works.
``evaluation/saliency.py`` turns that gradient into a picture.

``cut=True`` (not in the reference, whose graph is differentiated by TF as a whole): the backbone
runs under ``no_grad`` and ``grad_in`` is a leaf, so the gradient at the map costs a backward pass
of the head and nothing below it is kept for one.
"""
from . import nets


def vgg16Netvlad(image_batch, model=None, cut=False):
    """model/grad_nets.py:7-69.  image_batch [B,H,W,{1|3}] float, raw 0..255 RGB ->
    (descriptor [B, 32768], grad_in [B, h, w, 512])."""
    return (model or nets.default_model()).forward_with_map(image_batch, cut=cut)


def vgg16(image_batch, model=None, cut=False):
    """model/grad_nets.py:72-134 -> (channel-normalised conv5_3 map [B, h, w, 512], grad_in)."""
    return (model or nets.default_model()).forward_with_map(image_batch, vlad=False, cut=cut)
