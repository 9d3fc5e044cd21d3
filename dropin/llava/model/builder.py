from radvlm_amd.llava.model.builder import load_pretrained_model  # noqa: F401
