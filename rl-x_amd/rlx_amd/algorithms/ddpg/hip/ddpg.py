"""ddpg.hip -- DDPG (rl_x/algorithms/ddpg/flax/ddpg.py): td3.hip's host loop, acting and networks (ddpg/flax/policy.py is td3/flax's
file) with ONE critic (critic.py:17-30), no target-policy smoothing, no delay, and one joint loss whose two gradients are taken at
the same parameters (ddpg.py:114-166) -- rlx_td3_update_f32 with nr_critics = 1 and joint = 1 (rl-x_amd/csrc/td3.hip)."""
from rlx_amd.algorithms.ddpg.hip.general_properties import GeneralProperties
from rlx_amd.algorithms.td3.hip.td3 import TD3


class DDPG(TD3):
    _NAME = "ddpg.hip"
    NR_CRITICS, JOINT = 1, True

    def update_counters(self, nr_updates):
        return {"steps/nr_updates": self.nr_critic_updates}                  # ddpg.py:183, :247, :296: ONE counter

    def general_properties():
        return GeneralProperties
