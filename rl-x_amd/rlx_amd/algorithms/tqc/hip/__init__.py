"""`tqc.hip`: TQC (truncated quantile critics) whose update runs in librlxhip.so."""
from rlx_amd.plugin import register_algorithm_plugin
from . import default_config, general_properties
from .tqc import TQC

TQC_HIP = register_algorithm_plugin(__file__, default_config.get_config, TQC, general_properties.GeneralProperties)
