"""float64 reference of a generic geometry's training WITH decoder gradients: tests/generic_train_ref.py's forward with the state dict's decoder
tensors as float64 LEAVES next to the planes, so that torch.autograd gives d_natural -- the decoder's gradients in natural_blob order -- as
well.  A helper of tests/test_generic_train_decoder_fused.py, not a test.

generic_train_ref.forward reads a weight as torch.as_tensor(np.asarray(sd[key], np.float64)); torch.as_tensor hands a tensor through with its
graph, np.asarray does not take one that requires a gradient.  The forward is therefore run over the same code with a numpy whose asarray
leaves torch tensors alone (_KeepTensors); every other name of its module is what it was."""
import types

import numpy as np
import torch

import generic_train_ref as ref


class _KeepTensors:
    """numpy, but asarray(tensor, ...) is the tensor itself"""

    def __getattr__(self, name):
        return getattr(np, name)

    @staticmethod
    def asarray(v, *a, **k):
        return v if isinstance(v, torch.Tensor) else np.asarray(v, *a, **k)


_forward = types.FunctionType(ref.forward.__code__, dict(vars(ref), np=_KeepTensors()), "forward", ref.forward.__defaults__)


def natural_keys(dec_density_layers, dec_rgb_layers):
    """the state-dict keys of the decoder in natural_blob order: density layers, fc_alpha, rgb layers, fc_rgb; weight then bias"""
    keys = []
    for name, layers, head in (("density_dec", dec_density_layers, "fc_alpha"), ("rgb_dec", dec_rgb_layers, "fc_rgb")):
        for l in range(layers):
            keys += ["%s.0.%d.weight" % (name, l), "%s.0.%d.bias" % (name, l)]
        keys += [head + ".0.weight", head + ".0.bias"]
    return keys


def gradients(sd, planes, box, x, cotangent, dec_density_layers=4, dec_rgb_layers=4, **kw):
    """-> (out [P,4], d_natural [floats of the natural blob], [d plane as [1,C,H,W]]) of sum(out * cotangent), all float64 numpy"""
    keys = natural_keys(dec_density_layers, dec_rgb_layers)
    sd = dict(sd)
    for k in keys:
        sd[k] = torch.as_tensor(np.asarray(sd[k], np.float64)).clone().requires_grad_(True)
    leaves = [torch.as_tensor(np.asarray(p, np.float64)).clone().requires_grad_(True) for p in planes]
    out = _forward(sd, leaves, box, x, dec_density_layers=dec_density_layers, dec_rgb_layers=dec_rgb_layers, **kw)
    if out.shape[0]:
        (out * torch.as_tensor(np.asarray(cotangent, np.float64))).sum().backward()
    grad = lambda t: np.zeros(tuple(t.shape)) if t.grad is None else t.grad.numpy()
    return out.detach().numpy(), np.concatenate([grad(sd[k]).reshape(-1) for k in keys]), [grad(p) for p in leaves]


rel_l2 = ref.rel_l2
