"""`reppo.hip` flags = rl_x/algorithms/reppo/pytorch/default_config.py.  `compile_mode` has no meaning here (nothing is traced);
`bf16_mixed_precision_training` defaults to False: the library computes in fp32 (True is refused, not emulated);
`threefry_partitionable` selects the counter-RNG scheme of the library's noise draws (the reference uses torch's generator)."""
from rlx_amd.plugin import flag_namespace

FLAGS = dict(
    device="gpu", compile_mode="none", bf16_mixed_precision_training=False, total_timesteps=1000000000, learning_rate=3e-4,
    anneal_learning_rate=False, nr_steps=128, nr_epochs=4, nr_minibatches=128, gamma=0.99, gae_lambda=0.95, max_grad_norm=0.5,
    policy_hidden_dim=512, critic_hidden_dim=512, policy_min_std=0.0, nr_bins=151, v_min=-100.0, v_max=100.0,
    init_kl_coefficient=0.01, kl_bound=0.1, init_entropy_coefficient=0.01, target_entropy_multiplier=0.5,
    auxiliary_loss_coefficient=1.0, nr_kl_samples=16, normalize_observation=True, evaluation_frequency=-1, evaluation_episodes=10,
    threefry_partitionable=True,
)


def get_config(algorithm_name):
    return flag_namespace(algorithm_name, FLAGS)
