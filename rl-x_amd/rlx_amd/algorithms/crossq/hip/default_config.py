"""`crossq.hip` flags = rl_x/algorithms/crossq/flax/default_config.py (+ threefry_partitionable)."""
from rlx_amd.plugin import flag_namespace

FLAGS = dict(
    device="gpu", total_timesteps=1e9, learning_rate=1e-3, anneal_learning_rate=False,
    policy_adam_b1=0.5, critic_adam_b1=0.5,
    # replay
    buffer_size=10e6, learning_starts=5000, batch_size=256,
    # objective: no target networks, no tau; the policy is updated when global_step % policy_delay == 0
    gamma=0.99, ensemble_size=2, policy_delay=3,
    target_entropy="auto", log_std_min=-20, log_std_max=2,
    # batch renormalisation in front of every Dense of both networks
    batch_renorm_momentum=0.99, batch_renorm_warmup_steps=100000,
    policy_nr_hidden_units=256, critic_nr_hidden_units=2048,
    logging_frequency=3000, evaluation_frequency=-1, evaluation_episodes=10,
    threefry_partitionable=True,
)


def get_config(algorithm_name):
    return flag_namespace(algorithm_name, FLAGS)
