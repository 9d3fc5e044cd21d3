from radvlm_amd.llava.train.llava_trainer import *  # noqa: F401,F403
from radvlm_amd.llava.train.dpo_trainer import LLaVADPOTrainer  # noqa: F401  (the reference keeps it in this module)
