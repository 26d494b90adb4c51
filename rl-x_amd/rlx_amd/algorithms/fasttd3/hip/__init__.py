"""`fasttd3.hip`: FastTD3 (distributional twin critics, ReLU networks, deterministic tanh policy, AdamW) whose update runs in librlxhip.so."""
from rlx_amd.plugin import register_algorithm_plugin
from . import default_config, general_properties
from .fasttd3 import FastTD3

FASTTD3_HIP = register_algorithm_plugin(__file__, default_config.get_config, FastTD3, general_properties.GeneralProperties)
