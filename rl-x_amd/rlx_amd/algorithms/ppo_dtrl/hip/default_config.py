"""`ppo_dtrl.hip` flags = rl_x/algorithms/ppo_dtrl/flax_full_jit/default_config.py:10-32.  `nr_parallel_seeds` above 1 is refused.  The
last group is this build's own."""
from rlx_amd.plugin import flag_namespace

FLAGS = dict(
    device="gpu", nr_parallel_seeds=1, total_timesteps=2e9, learning_rate=4e-4, anneal_learning_rate=True, nr_steps=128, nr_epochs=10,
    minibatch_size=32768, gamma=0.99, gae_lambda=0.9, clip_range=0.1, entropy_coef=0.0, critic_coef=1.0, max_grad_norm=5.0, std_dev=1.0,
    mean_bound=0.03, cov_bound=0.001, trust_region_coef=0.1, action_clipping_and_rescaling=False,
    evaluation_and_save_frequency=17301504, evaluation_active=False,
    # ---- this build
    evaluation_episodes=10,            # episodes of one evaluation (the reference runs one horizon of its vectorised eval env)
    threefry_partitionable=True,       # key schedule of the acting noise and the minibatch permutation (as ppo.hip)
    fused_rollout=True,                # one kernel per acting step when the network shapes allow it (as ppo.hip)
)


def get_config(algorithm_name):
    return flag_namespace(algorithm_name, FLAGS)
