"""`mpo.hip` flags = rl_x/algorithms/mpo/pytorch/default_config.py:7-49.  `compile_mode` has no meaning here (nothing is traced);
`bf16_mixed_precision_training` defaults to False: the library computes in fp32 (True is refused, not emulated)."""
from rlx_amd.plugin import flag_namespace

FLAGS = dict(
    device="gpu", compile_mode="none", bf16_mixed_precision_training=False, total_timesteps=1e9, agent_learning_rate=3e-4,
    dual_learning_rate=1e-2, anneal_agent_learning_rate=False, anneal_dual_learning_rate=False, buffer_size=1e6, learning_starts=5000,
    batch_size=256, actor_update_period=1000, target_network_update_period=100, gamma=0.99, n_steps=4, optimize_every_n_steps=4,
    action_sampling_number=20, max_grad_norm=40.0, epsilon_non_parametric=0.1, epsilon_parametric_mu=0.01, epsilon_parametric_sigma=1e-6,
    epsilon_penalty=0.001, init_log_eta=10.0, init_log_alpha_mean=10.0, init_log_alpha_stddev=1000.0, init_log_penalty_temperature=10.0,
    policy_init_scale=0.5, policy_min_scale=1e-6, action_clipping=True, action_rescaling=True, v_min=-1600.0, v_max=1600.0, nr_atoms=51,
    nr_hidden_units=256, float_epsilon=1e-8, min_log_temperature=-18.0, min_log_alpha=-18.0, enable_observation_normalization=True,
    logging_frequency=300, evaluation_frequency=-1, evaluation_episodes=10,
    threefry_partitionable=True,
)


def get_config(algorithm_name):
    return flag_namespace(algorithm_name, FLAGS)
