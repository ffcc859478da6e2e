"""Parameters of the g24 models (the positional-encoding NeRF baseline), shared by gen_golden_pe.py and the tests.

The two FlexibleNeRFModel(num_encoding_fn_xyz=6, num_encoding_fn_dir=4, include_input_xyz=True, include_input_dir=True) instances of g24 are
not stored: their parameters come from numpy's legacy RandomState, whose stream does not change between versions -- uniform(-1/sqrt(fan_in),
1/sqrt(fan_in)) per tensor, like nn.Linear's default, in state-dict order.  Gradients and post-Adam parameters (81 476 floats per model) are
stored at mip_params.kept_elements(name, numel), the rule g23 uses."""
import mip_params
from mip_params import KEEP, checksum, kept, kept_elements  # noqa: F401  (re-exported: the tests read them from here)

# state-dict order of FlexibleNeRFModel(include_input_xyz=True) with the constructor defaults: (name, shape)
SHAPES = [("layer1.weight", (128, 39))] + mip_params.SHAPES[1:]
SEEDS = (303, 404)       # coarse, fine


def state_dict(seed):
    """{name: float32 array} of the model with this seed"""
    return mip_params.state_dict(seed, SHAPES)
