from .config import (DPOConfig, GKDConfig, GRPOConfig, RewardConfig, SFTConfig, apply_overrides, config_from_env,
                     load_config_file)
from .callbacks import (TrainerCallback, TrainerControl, TrainerState, TrainingHistoryCallback, PerplexityCallback,
                        AimCallback, JSONLLoggerCallback)
from .trainer import SFTTrainer, TrainOutput, set_seed
from .dpo import DPOTrainer
from .gkd import GKDTrainer
from .grpo import GRPOTrainer
from .reward import RewardTrainer

__all__ = ["SFTConfig", "config_from_env", "TrainerCallback", "TrainerControl", "TrainerState",
           "TrainingHistoryCallback", "PerplexityCallback", "AimCallback", "JSONLLoggerCallback", "SFTTrainer",
           "TrainOutput", "set_seed", "DPOConfig", "DPOTrainer", "GKDConfig", "GKDTrainer",
           "GRPOConfig", "GRPOTrainer", "RewardConfig", "RewardTrainer"]
