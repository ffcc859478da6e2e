"""Parameters of the g24 models (the positional-encoding NeRF baseline), shared by gen_golden_pe.py and the tests.

The two FlexibleNeRFModel(num_encoding_fn_xyz=6, num_encoding_fn_dir=4, include_input_xyz=True, include_input_dir=True) instances of g24 are
not stored: their parameters come from numpy's legacy RandomState, whose stream does not change between versions -- uniform(-1/sqrt(fan_in),
1/sqrt(fan_in)) per tensor, like nn.Linear's default, in state-dict order.  Gradients and post-Adam parameters (81 476 floats per model) are
stored at mip_params.kept_elements(name, numel), the rule g23 uses."""
import numpy as np

from mip_params import KEEP, kept, kept_elements  # noqa: F401  (re-exported: the tests read them from here)

# state-dict order of FlexibleNeRFModel(include_input_xyz=True) with the constructor defaults: (name, shape)
SHAPES = [("layer1.weight", (128, 39)), ("layer1.bias", (128,))]
SHAPES += [x for j in range(3) for x in (("layers_xyz.%d.weight" % j, (128, 128)), ("layers_xyz.%d.bias" % j, (128,)))]
SHAPES += [("layers_dir.0.weight", (64, 155)), ("layers_dir.0.bias", (64,)), ("fc_alpha.weight", (1, 128)), ("fc_alpha.bias", (1,)),
           ("fc_rgb.weight", (3, 64)), ("fc_rgb.bias", (3,)), ("fc_feat.weight", (128, 128)), ("fc_feat.bias", (128,))]
SEEDS = (303, 404)       # coarse, fine


def state_dict(seed):
    """{name: float32 array} of the model with this seed"""
    rs = np.random.RandomState(seed)
    out = {}
    for name, shape in SHAPES:
        fan_in = dict(SHAPES)[name.rsplit(".", 1)[0] + ".weight"][1]
        b = 1.0 / np.sqrt(fan_in)
        out[name] = rs.uniform(-b, b, size=shape).astype(np.float32)
    return out


def checksum(sd):
    """float64 sum and sum of squares of every parameter: what the fixture stores in place of the parameters"""
    flat = np.concatenate([v.reshape(-1).astype(np.float64) for v in sd.values()])
    return np.array([flat.sum(), (flat * flat).sum()])
