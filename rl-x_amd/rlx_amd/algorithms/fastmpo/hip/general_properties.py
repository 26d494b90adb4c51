"""What `fastmpo.hip` can be paired with (rl_x/algorithms/fastmpo/flax_full_jit/general_properties.py; the reference's JAX data
interface is this project's device-resident TORCH one)."""
from rlx_amd.plugin import algorithm_properties

GeneralProperties = algorithm_properties(observations=("FLAT_VALUES",), actions=("CONTINUOUS",), interfaces=("TORCH",),
                                         framework="TORCH")
