"""`espo.hip` flags = rl_x/algorithms/espo/pytorch/default_config.py:7-29.  `compile_mode` has no meaning here (nothing is traced);
`bf16_mixed_precision_training` defaults to False: the library computes in fp32 (True is refused, not emulated).  The last group is
this build's own."""
from rlx_amd.plugin import flag_namespace

FLAGS = dict(
    device="gpu", compile_mode="none", bf16_mixed_precision_training=False, total_timesteps=1e9, learning_rate=3e-4,
    anneal_learning_rate=False, nr_steps=2048, max_epochs=300, minibatch_size=64, gamma=0.99, gae_lambda=0.95, max_ratio_delta=0.25,
    delta_calc_operator="mean", entropy_coef=0.0, critic_coef=0.5, max_grad_norm=0.5, std_dev=1.0, action_clipping_and_rescaling=True,
    nr_hidden_units=256, evaluation_frequency=-1, evaluation_episodes=10,
    # ---- this build
    threefry_partitionable=True,       # key schedule of the acting noise (as ppo.hip)
    fused_rollout=True,                # one kernel per acting step when the network shapes allow it (as ppo.hip)
)


def get_config(algorithm_name):
    return flag_namespace(algorithm_name, FLAGS)
