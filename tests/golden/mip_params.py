"""Parameters of the g23 models and the elements g23 keeps of every parameter-shaped array, shared by gen_golden_mip.py and the tests.

The two FlexibleNeRFModel(include_input_xyz=False) instances of g23 are not stored: their parameters come from numpy's legacy RandomState,
whose stream does not change between versions -- uniform(-1/sqrt(fan_in), 1/sqrt(fan_in)) per tensor, like nn.Linear's default, in
state-dict order.  Gradients and post-Adam parameters (81 092 floats per model) are stored at `kept_elements(name, numel)`: every element
of a tensor of up to KEEP elements, a fixed random KEEP of the larger ones."""
import zlib

import numpy as np

# state-dict order of FlexibleNeRFModel(include_input_xyz=False) with the constructor defaults: (name, shape)
SHAPES = [("layer1.weight", (128, 36)), ("layer1.bias", (128,))]
SHAPES += [x for j in range(3) for x in (("layers_xyz.%d.weight" % j, (128, 128)), ("layers_xyz.%d.bias" % j, (128,)))]
SHAPES += [("layers_dir.0.weight", (64, 155)), ("layers_dir.0.bias", (64,)), ("fc_alpha.weight", (1, 128)), ("fc_alpha.bias", (1,)),
           ("fc_rgb.weight", (3, 64)), ("fc_rgb.bias", (3,)), ("fc_feat.weight", (128, 128)), ("fc_feat.bias", (128,))]
KEEP = 1024
SEEDS = (101, 202)       # coarse, fine


def state_dict(seed, shapes=SHAPES):
    """{name: float32 array} of the model with this seed (`shapes`: pe_params.SHAPES for the g24 models)"""
    rs = np.random.RandomState(seed)
    out = {}
    for name, shape in shapes:
        fan_in = dict(shapes)[name.rsplit(".", 1)[0] + ".weight"][1]
        b = 1.0 / np.sqrt(fan_in)
        out[name] = rs.uniform(-b, b, size=shape).astype(np.float32)
    return out


def checksum(sd):
    """float64 sum and sum of squares of every parameter: what the fixtures store in place of the parameters"""
    flat = np.concatenate([v.reshape(-1).astype(np.float64) for v in sd.values()])
    return np.array([flat.sum(), (flat * flat).sum()])


def kept_elements(name, numel):
    """flat indices g23 stores of a tensor `name` with `numel` elements (sorted)"""
    if numel <= KEEP:
        return np.arange(numel)
    rs = np.random.RandomState(zlib.crc32(name.encode()))
    return np.sort(rs.choice(numel, KEEP, replace=False))


def kept(name, array):
    a = np.asarray(array).reshape(-1)
    return a[kept_elements(name, a.size)]
