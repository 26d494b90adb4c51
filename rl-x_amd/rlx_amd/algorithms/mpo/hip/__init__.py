"""`mpo.hip`: MPO (distributional critic, non-parametric E-step, decoupled Gaussian M-step, dual variables) whose update runs in librlxhip.so."""
from rlx_amd.plugin import register_algorithm_plugin
from . import default_config, general_properties
from .mpo import MPO

MPO_HIP = register_algorithm_plugin(__file__, default_config.get_config, MPO, general_properties.GeneralProperties)
