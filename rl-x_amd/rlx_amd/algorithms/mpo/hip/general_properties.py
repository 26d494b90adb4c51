"""What `mpo.hip` can be paired with (rl_x/algorithms/mpo/pytorch/general_properties.py)."""
from rlx_amd.plugin import algorithm_properties

GeneralProperties = algorithm_properties(observations=("FLAT_VALUES",), actions=("CONTINUOUS",), interfaces=("NUMPY", "TORCH"),
                                         framework="TORCH")
