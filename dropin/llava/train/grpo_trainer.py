from radvlm_amd.llava.train.grpo_trainer import *  # noqa: F401,F403
from radvlm_amd.llava.train.grpo_trainer import GRPOTrainer  # noqa: F401
