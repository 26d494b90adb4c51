from rlx_amd.hip.lib import (  # noqa: F401
    load_library, library_path, RlxError, Ctx, MlpDesc, PpoHparams, SacHparams, mlp_desc, LnMlpDesc, FastSacHparams, lnmlp_desc,
    FastTd3Hparams, relu_mlp_desc, ReppoDesc, ReppoHparams, reppo_desc, MpoDesc, MpoHparams, mpo_desc, EspoHparams, TqcHparams,
    RedqHparams, redq_subset, Td3Hparams, AqeHparams, DroqHparams, FastMpoDesc, FastMpoHparams, fastmpo_desc,
    ACT_TANH, ACT_ELU, ACT_RELU, THREEFRY_LEGACY, THREEFRY_PARTITIONABLE,
)
