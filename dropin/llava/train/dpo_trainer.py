from radvlm_amd.llava.train.dpo_trainer import *  # noqa: F401,F403
from radvlm_amd.llava.train.dpo_trainer import DPODataCollator, DPODataset, LLaVADPOTrainer  # noqa: F401
