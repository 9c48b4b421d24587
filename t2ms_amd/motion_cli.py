"""What the motion drivers (myinfer.py, mytrain.py) share on their command lines: the values the reference keeps in
config.yaml as flags, `--config FILE` for those who have PyYAML, the per-dataset defaults and the reference's path formats.
Host-only; no kernel is involved."""
import os

from datafactory.motion import DEFAULTS

# config.yaml's feature names; the last input_dim of them are the channels
FEATURES = {
    "benchpress": ["bar_x", "bar_y", "barx/bar_y", "left_shoulder_y", "right_shoulder_y", "left_dist", "right_dist", "left_elbow",
                   "left_shoulder", "right_elbow", "right_shoulder", "left_torso-arm", "right_torso-arm"],
    "deadlift": ["bar_x", "bar_y", "left_knee", "left_hip", "right_knee", "right_hip", "body_length", "left_torso-arm",
                 "right_torso-arm"],
}
PRETRAINED_EPC = {"benchpress": 16000, "deadlift": 20000}
PRETRAINED_ROOT = "./results/saved_pretrained_models"


def from_yaml(args, prog):
    """--config FILE, when PyYAML is importable and the file exists: the values the reference's get_cfg reads."""
    if not args.config or not os.path.exists(args.config):
        return {}
    try:
        import yaml
    except ImportError:
        print(f"{prog}: PyYAML is not installed, {args.config} is not read (flags and built-in defaults hold)")
        return {}
    with open(args.config, "r", encoding="utf-8") as f:
        config = yaml.safe_load(f)
    cfg = config[args.dataset_name]
    out = dict(dataset_root=config.get("dataset_root"), general_seed=config.get("general_seed"),
               features=[f[0]["name"] for f in cfg["features"].values()], flow_dim=cfg.get("flow_dim"), input_dim=cfg.get("input_dim"),
               split_base_num=cfg["dataset"].get("split_base_num"), caption=cfg["dataset"].get("caption"),
               pretrained_epc=cfg["vae"].get("epoch"), denoiser=cfg["diffusion"].get("denoiser"),
               backbone=cfg["diffusion"].get("backbone"))
    for k in ("block_hidden_size", "num_residual_layers", "res_hidden_size", "embedding_dim"):
        out[k] = cfg["vae"].get(k)
    return {k: v for k, v in out.items() if v is not None}


def add_config_flags(p):
    """config.yaml's values, as flags (None: the dataset's default) -- and the two switches every motion driver has."""
    p.add_argument("--config", type=str, default="config.yaml", help="model configuration (read only when PyYAML is installed)")
    p.add_argument("--dataset_root", type=str, default=None)
    p.add_argument("--general_seed", type=int, default=None)
    p.add_argument("--caption", type=str, default=None)
    p.add_argument("--split_base_num", type=int, default=None)
    p.add_argument("--input_dim", type=int, default=None)
    p.add_argument("--flow_dim", type=int, default=None)
    p.add_argument("--pretrained_epc", type=int, default=None)
    p.add_argument("--block_hidden_size", type=int, default=None)
    p.add_argument("--num_residual_layers", type=int, default=None)
    p.add_argument("--res_hidden_size", type=int, default=None)
    p.add_argument("--embedding_dim", type=int, default=None)
    p.add_argument("--backbone", type=str, choices=["flowmatching", "ddpm"], default=None)
    p.add_argument("--denoiser", type=str, choices=["DiT"], default=None)
    p.add_argument("--embedding", choices=["summary", "prefix"], default="summary", help="bench press: which stored embedding conditions a clip")
    p.add_argument("--random_init", action="store_true", help="seeded synthetic weights instead of checkpoints")


def resolve(args, prog):
    """Fill every config value a flag left open (file first, then the built-in per-dataset default) and the paths both
    drivers share: args.features, args.pretrainedvae_path, args.checkpoint_dir."""
    name = args.dataset_name
    builtin = dict(DEFAULTS[name], dataset_root="./Data", general_seed=2025, pretrained_epc=PRETRAINED_EPC[name], block_hidden_size=128,
                   num_residual_layers=3, res_hidden_size=256, embedding_dim=64, backbone="flowmatching", denoiser="DiT")
    from_file = from_yaml(args, prog)
    for k, v in builtin.items():
        if getattr(args, k) is None:
            setattr(args, k, from_file.get(k, v))
    args.features = from_file.get("features", FEATURES[name])
    # the reference's paths (myinfer.py:240-243, mytrain.py:115-116)
    args.pretrainedvae_path = os.path.join(PRETRAINED_ROOT, f"{args.split_base_num}_{name}_epoch{args.pretrained_epc}", "final_model.pth")
    args.checkpoint_dir = os.path.join(args.save_path, "checkpoints", "{}_{}_{}_{}_{}".format(
        args.backbone, args.denoiser, name, args.caption, args.pretrained_epc))
    return args


def checkpoint_file(args, epoch):
    """The denoiser checkpoint mytrain.py writes after `epoch` and myinfer.py --checkpoint_id `epoch` loads."""
    return os.path.join(args.checkpoint_dir, "model_{}.pth".format(epoch))


def embedding_index(record_len, embedding):
    """Which field of a loader record (text, x, *embeddings, subject) conditions a clip: deadlift stores one embedding,
    bench press two (prefix, then summary)."""
    return 2 if record_len == 4 or embedding == "prefix" else 3
