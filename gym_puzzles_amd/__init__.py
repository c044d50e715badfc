"""gym_puzzles_amd -- MI355X-native MultiRobotPuzzle step (HIP/gfx950) behind the
gym_puzzles env interface.  See DESIGN.md.

    Batch                  N lanes on one GPU, thin wrapper of the C ABI (include/mrp.h)
    envs.MultiRobotPuzzle  gym-style single env classes (same names as gym_puzzles.envs)
    envs.make(id)          gym.make equivalent (adds gym 0.21's TimeLimit)
    MultiRobotPuzzleVecEnv SB3-style vectorised env with on-device auto-reset
    MultiRobotPuzzleVecNormalize / DeviceVecNormalize
                           SB3 VecNormalize + Monitor statistics on the device
    pixels                 the numpy restatement of the pixel observations (Batch.pixels, obs_type="image")
    DeviceRolloutBuffer    SB3 RolloutBuffer on the device: TimeLimit bootstrap + GAE in one launch
                           (rollout.gae_device; rollout.gae_ref is the numpy restatement of the rule)
    DevicePolicy           SB3 ActorCriticPolicy (MlpExtractor) on the device: forward, sampling, log-prob, value
                           and clipping in one launch (policy.policy_ref / tanh_ref state the rule in numpy);
                           rollout.collect_rollouts runs act / step / normalise / add without a host sync
    DevicePPO              one optimiser step of SB3's PPO.train() on the device -- evaluate_actions, losses,
                           backward, grad-norm clip, Adam -- writing the DevicePolicy's parameters in place
                           (ppo.ppo_grad_ref / adam_ref / ppo_train_ref / exp_ref state the rule in numpy), with
                           SB3's clip_range_vf and target_kl (ppo.kl_stop_ref) and, with minibatch="device", the
                           minibatch gather and advantage normalisation (ppo.normalize_adv_ref) in HIP; with a
                           dist.Shard / dist.GradExchange, data-parallel training: the ranks' gradients combined
                           in rank order, clip and Adam on the device (ppo.combine_ref / ppo_train_dist_ref)
"""
from ._native import ENV_IDS, Batch, MrpError, env_dims  # noqa: F401
from .policy import policy_ref, tanh_ref  # noqa: F401  (pure numpy)
from .ppo import (adam_ref, combine_ref, exp_ref, kl_stop_ref, normalize_adv_ref, ppo_grad_ref,  # noqa: F401  (pure numpy)
                  ppo_train_dist_ref, ppo_train_ref)


def __getattr__(name):
    # the env classes import lazily so that `import gym_puzzles_amd` never touches the GPU
    if name in ("MultiRobotPuzzle", "MultiRobotPuzzleHeavy", "MultiRobotPuzzle2", "MultiRobotPuzzleHeavy2",
                "MultiRobotPuzzleHeavy2ThreeBlock", "RobotPuzzleBase", "make"):
        from . import envs
        return getattr(envs, name)
    if name in ("MultiRobotPuzzleVecEnv", "MultiRobotPuzzleVecNormalize", "DeviceVecNormalize"):
        from . import vec_env
        return getattr(vec_env, name)
    if name == "DeviceRolloutBuffer":
        from . import rollout
        return rollout.DeviceRolloutBuffer
    if name == "DevicePolicy":
        from . import policy
        return policy.DevicePolicy
    if name == "DevicePPO":
        from . import ppo
        return ppo.DevicePPO
    if name == "collect_rollouts":
        from . import rollout
        return rollout.collect_rollouts
    raise AttributeError(name)
