"""`espo.hip`: ESPO (policy optimisation with early stopping on the ratio deviation) whose epoch loop runs in librlxhip.so."""
from rlx_amd.plugin import register_algorithm_plugin
from . import default_config, general_properties
from .espo import ESPO

ESPO_HIP = register_algorithm_plugin(__file__, default_config.get_config, ESPO, general_properties.GeneralProperties)
