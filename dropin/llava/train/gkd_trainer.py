from radvlm_amd.llava.train.gkd_trainer import *  # noqa: F401,F403
from radvlm_amd.llava.train.gkd_trainer import GKDTrainer  # noqa: F401
