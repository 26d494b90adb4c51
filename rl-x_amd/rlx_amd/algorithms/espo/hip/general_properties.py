"""What `espo.hip` can be paired with (rl_x/algorithms/espo/pytorch/general_properties.py): flat observations, continuous actions,
a device-resident (TORCH) environment."""
from rlx_amd.plugin import algorithm_properties

GeneralProperties = algorithm_properties(observations=("FLAT_VALUES",), actions=("CONTINUOUS",), interfaces=("TORCH",), framework="TORCH")
