"""Merge the adapters of a LoRA run into its base model and save a full checkpoint (LLaVA's "merge and save" step).

  python tools/merge_lora.py --model-path RUN_DIR --model-base BASE_DIR --save-model-path OUT_DIR

RUN_DIR is what --lora_enable training saved (adapter_config.json, adapter_model.bin, non_lora_trainables.bin, config.json); BASE_DIR
a full checkpoint of the base model.  OUT_DIR receives config.json + model.safetensors under the reference names, which
load_pretrained_model(OUT_DIR) loads without a model_base.  --model-base may be omitted when the adapter config's
base_model_name_or_path is a local directory."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--model-path", required=True)
    ap.add_argument("--model-base", default=None)
    ap.add_argument("--save-model-path", required=True)
    ap.add_argument("--device", default="cuda")
    a = ap.parse_args(argv)
    from radvlm_amd.llava.model.builder import load_pretrained_model
    tokenizer, model, _, _ = load_pretrained_model(a.model_path, model_base=a.model_base, device=a.device)
    model.save_pretrained(a.save_model_path)
    if tokenizer is not None:
        tokenizer.save_pretrained(a.save_model_path)
    print(f"merged {a.model_path} into {a.model_base or 'its base model'}: {a.save_model_path}", flush=True)


if __name__ == "__main__":
    main()
