"""`fasttd3.hip` flags = rl_x/algorithms/fasttd3/pytorch/default_config.py:9-38.  `compile_mode` has no meaning here (nothing is
traced); `bf16_mixed_precision_training` defaults to False: the library computes in fp32 (True is refused, not emulated)."""
from rlx_amd.plugin import flag_namespace

FLAGS = dict(
    device="gpu", compile_mode="none", bf16_mixed_precision_training=False, total_timesteps=2000158720, learning_rate=3e-4,
    anneal_learning_rate=False, weight_decay=0.1,
    # replay
    batch_size=32768, buffer_size_per_env=10240, learning_starts=10, n_steps=1,
    # objective
    v_min=-10.0, v_max=10.0, tau=0.1, gamma=0.97, nr_atoms=101,
    noise_std_min=0.001, noise_std_max=0.4, smoothing_epsilon=0.001, smoothing_clip_value=0.5,
    nr_critic_updates_per_policy_update=2, nr_policy_updates_per_step=1, clipped_double_q_learning=True, max_grad_norm=-1.0,
    action_clipping_and_rescaling=False, enable_observation_normalization=True,
    logging_frequency=40960, evaluation_frequency=-1, save_frequency=4096000,
    threefry_partitionable=True,
)


def get_config(algorithm_name):
    return flag_namespace(algorithm_name, FLAGS)
