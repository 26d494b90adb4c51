"""`td3.hip`: TD3 (twin delayed deep deterministic policy gradients) whose update runs in librlxhip.so."""
from rlx_amd.plugin import register_algorithm_plugin
from . import default_config, general_properties
from .td3 import TD3

TD3_HIP = register_algorithm_plugin(__file__, default_config.get_config, TD3, general_properties.GeneralProperties)
