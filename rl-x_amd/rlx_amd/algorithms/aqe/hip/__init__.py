"""`aqe.hip`: AQE (truncated-mean multi-head ensemble critics) whose update runs in librlxhip.so."""
from rlx_amd.plugin import register_algorithm_plugin
from . import default_config, general_properties
from .aqe import AQE

AQE_HIP = register_algorithm_plugin(__file__, default_config.get_config, AQE, general_properties.GeneralProperties)
