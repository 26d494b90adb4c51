"""`reppo.hip`: REPPO (on-policy rollouts, soft TD-lambda targets, HL-Gauss critic, pathwise policy with a KL trust region) whose
acting, targets and update run in librlxhip.so."""
from rlx_amd.plugin import register_algorithm_plugin
from . import default_config, general_properties
from .reppo import REPPO

REPPO_HIP = register_algorithm_plugin(__file__, default_config.get_config, REPPO, general_properties.GeneralProperties)
