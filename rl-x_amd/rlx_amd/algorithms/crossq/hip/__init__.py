"""`crossq.hip`: CrossQ (batch-renormalised critics, no target networks) whose updates run in librlxhip.so."""
from rlx_amd.plugin import register_algorithm_plugin
from . import default_config, general_properties
from .crossq import CrossQ

CROSSQ_HIP = register_algorithm_plugin(__file__, default_config.get_config, CrossQ, general_properties.GeneralProperties)
