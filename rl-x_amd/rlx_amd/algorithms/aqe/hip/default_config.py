"""`aqe.hip` flags = rl_x/algorithms/aqe/flax/default_config.py:9-28 (+ threefry_partitionable)."""
from rlx_amd.plugin import flag_namespace

FLAGS = dict(
    device="gpu", total_timesteps=1e9, learning_rate=3e-4, anneal_learning_rate=False,
    # replay
    buffer_size=1e6, learning_starts=5000, batch_size=256,
    # objective
    tau=0.005, gamma=0.99,
    # critics: ensemble_size nets with nr_heads_per_net outputs each; every critic step pools all their target values, drops the
    # nr_dropped_q_values largest of the pool and takes the mean of the rest; q_update_steps critic steps on fresh batches per
    # policy step
    ensemble_size=10, nr_heads_per_net=2, nr_dropped_q_values=4, q_update_steps=5,
    target_entropy="auto", log_std_min=-20, log_std_max=2,
    nr_hidden_units=256,
    logging_frequency=300, evaluation_frequency=-1, evaluation_episodes=10,
    threefry_partitionable=True,
)


def get_config(algorithm_name):
    return flag_namespace(algorithm_name, FLAGS)
