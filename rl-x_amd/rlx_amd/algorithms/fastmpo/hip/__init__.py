"""`fastmpo.hip`: FastMPO (one or two categorical critics, MPO's E-step / M-step / dual step, AdamW, Polyak targets) whose update runs in librlxhip.so."""
from rlx_amd.plugin import register_algorithm_plugin
from . import default_config, general_properties
from .fastmpo import FastMPO

FASTMPO_HIP = register_algorithm_plugin(__file__, default_config.get_config, FastMPO, general_properties.GeneralProperties)
