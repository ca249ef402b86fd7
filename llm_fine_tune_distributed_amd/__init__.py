"""MI355X-native distributed SFT framework (capabilities of thesteve0/llm-fine-tune-distributed).

Public API mirrors the reference's TRL surface: ``SFTConfig`` + ``SFTTrainer(...).train()``, and for preference
training ``DPOConfig`` + ``DPOTrainer(...).train()``, for knowledge distillation ``GKDConfig`` +
``GKDTrainer(..., teacher_model=...).train()``, for reinforcement learning from reward functions ``GRPOConfig`` +
``GRPOTrainer(model, reward_funcs, ...).train()``, for reward modelling on preference pairs ``RewardConfig`` +
``RewardTrainer(...).train()`` (its models are also ``GRPOTrainer`` reward functions).
"""
__version__ = "0.1.0"

from .models import ModelConfig, CausalLM, build_model, get_config  # noqa: F401


def __getattr__(name):
    # lazy imports keep `import llm_fine_tune_distributed_amd` light for the launcher
    if name in ("SFTConfig",):
        from .train.config import SFTConfig
        return SFTConfig
    if name in ("DPOConfig",):
        from .train.config import DPOConfig
        return DPOConfig
    if name in ("DPOTrainer",):
        from .train.dpo import DPOTrainer
        return DPOTrainer
    if name in ("GKDConfig",):
        from .train.config import GKDConfig
        return GKDConfig
    if name in ("GKDTrainer",):
        from .train.gkd import GKDTrainer
        return GKDTrainer
    if name in ("GRPOConfig",):
        from .train.config import GRPOConfig
        return GRPOConfig
    if name in ("GRPOTrainer",):
        from .train.grpo import GRPOTrainer
        return GRPOTrainer
    if name in ("RewardConfig",):
        from .train.config import RewardConfig
        return RewardConfig
    if name in ("RewardTrainer",):
        from .train.reward import RewardTrainer
        return RewardTrainer
    if name in ("SFTTrainer", "TrainOutput"):
        from .train import trainer
        return getattr(trainer, name)
    if name in ("TrainerCallback",):
        from .train.callbacks import TrainerCallback
        return TrainerCallback
    raise AttributeError(name)
