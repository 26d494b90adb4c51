"""`droq.hip`: DroQ (dropout Q-functions) whose update runs in librlxhip.so."""
from rlx_amd.plugin import register_algorithm_plugin
from . import default_config, general_properties
from .droq import DroQ

DROQ_HIP = register_algorithm_plugin(__file__, default_config.get_config, DroQ, general_properties.GeneralProperties)
