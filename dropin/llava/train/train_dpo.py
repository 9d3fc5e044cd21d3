from radvlm_amd.llava.train.train_dpo import *  # noqa: F401,F403
from radvlm_amd.llava.train.train_dpo import train  # noqa: F401

if __name__ == "__main__":
    train()
