"""`tqc.hip` flags = rl_x/algorithms/tqc/flax/default_config.py:9-28 (+ threefry_partitionable)."""
from rlx_amd.plugin import flag_namespace

FLAGS = dict(
    device="gpu", total_timesteps=1e9, learning_rate=3e-4, anneal_learning_rate=False,
    # replay
    buffer_size=1e6, learning_starts=5000, batch_size=256,
    # objective
    tau=0.005, gamma=0.99,
    # critics: ensemble_size nets of nr_atoms_per_net quantiles; the target drops the nr_dropped_atoms_per_net * ensemble_size
    # largest of the pooled next-state atoms
    ensemble_size=2, nr_atoms_per_net=25, nr_dropped_atoms_per_net=2, huber_kappa=1.0,
    target_entropy="auto", log_std_min=-20.0, log_std_max=2.0,
    nr_hidden_units=256,
    logging_frequency=3000, evaluation_frequency=-1, evaluation_episodes=10,
    threefry_partitionable=True,
)


def get_config(algorithm_name):
    return flag_namespace(algorithm_name, FLAGS)
