"""`fastmpo.hip` flags = rl_x/algorithms/fastmpo/flax_full_jit/default_config.py:9-61, value by value."""
from rlx_amd.plugin import flag_namespace

FLAGS = dict(
    device="gpu", nr_parallel_seeds=1, total_timesteps=2000158720, critic_network_type="fastsac", dual_critic=True,
    policy_network_type="fastsac", action_clipping=False, action_rescaling="none", policy_learning_rate=3e-4, critic_learning_rate=3e-4,
    dual_learning_rate=1e-2, anneal_policy_learning_rate=False, anneal_critic_learning_rate=False, anneal_dual_learning_rate=False,
    policy_weight_decay=0.001, critic_weight_decay=0.001, dual_weight_decay=0.0, adam_beta1=0.9, adam_beta2=0.95, max_grad_norm=40.0,
    collect_data_with_online_policy=False, action_sampling_number=4, epsilon_non_parametric=0.1, epsilon_parametric_mu=0.01,
    epsilon_parametric_sigma=1e-6, epsilon_penalty=0.001, init_log_eta=10.0, init_log_alpha_mean=10.0, init_log_alpha_stddev=1000.0,
    init_log_penalty_temperature=10.0, float_epsilon=1e-8, min_log_temperature=-18.0, min_log_alpha=-18.0, policy_init_scale=0.5,
    policy_min_scale=0.1, batch_size=8192, buffer_size_per_env=1024, learning_starts=10, v_min=-20.0, v_max=20.0, critic_tau=0.125,
    policy_tau=0.3, gamma=0.97, nr_atoms=101, n_steps=1, clipped_double_q_learning=False, nr_critic_updates_per_policy_update=4,
    nr_policy_updates_per_step=2, enable_observation_normalization=True, normalizer_epsilon=1e-8, logging_frequency=40960,
    evaluation_and_save_frequency=18350080, evaluation_active=False,
    threefry_partitionable=True,
)


def get_config(algorithm_name):
    return flag_namespace(algorithm_name, FLAGS)
