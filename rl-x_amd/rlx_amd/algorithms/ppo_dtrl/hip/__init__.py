"""`ppo_dtrl.hip`: PPO with differentiable trust-region layers whose update loop runs in librlxhip.so (rl-x_amd/csrc/dtrl.hip)."""
from rlx_amd.plugin import register_algorithm_plugin
from . import default_config, general_properties
from .ppo_dtrl import PPODTRL

PPO_DTRL_HIP = register_algorithm_plugin(__file__, default_config.get_config, PPODTRL, general_properties.GeneralProperties)
