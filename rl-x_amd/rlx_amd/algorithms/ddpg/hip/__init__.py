"""`ddpg.hip`: DDPG (deep deterministic policy gradients) whose update runs in librlxhip.so."""
from rlx_amd.plugin import register_algorithm_plugin
from . import default_config, general_properties
from .ddpg import DDPG

DDPG_HIP = register_algorithm_plugin(__file__, default_config.get_config, DDPG, general_properties.GeneralProperties)
