"""`redq.hip`: REDQ (randomized ensembled double Q-learning) whose update runs in librlxhip.so."""
from rlx_amd.plugin import register_algorithm_plugin
from . import default_config, general_properties
from .redq import REDQ

REDQ_HIP = register_algorithm_plugin(__file__, default_config.get_config, REDQ, general_properties.GeneralProperties)
