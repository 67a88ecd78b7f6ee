"""`run-smart-tree` entry point (reference smart_tree/cli.py:10-26) without hydra: the YAML `_target_`
tree is instantiated by a small recursive loader, `+path=...` / `+directory=...` and `a.b=value`
overrides are accepted on the command line (smart_tree_amd/config.py)."""
from __future__ import annotations

import sys
from pathlib import Path

from .config import apply_overrides, instantiate, load_yaml  # noqa: F401  (instantiate: part of this module's interface)


def load_config(overrides=()):
    return apply_overrides(load_yaml(Path(__file__).resolve().parent / "conf" / "pipeline.yaml"), overrides)


def main(argv=None):
    cfg = load_config(argv if argv is not None else sys.argv[1:])
    pipeline = instantiate(cfg["pipeline"])
    if "path" in cfg:
        pipeline.process_cloud(Path(cfg["path"]))
    elif "directory" in cfg:  # every entry of the directory, as cli.py:22-23 (sorted; files load_cloud cannot read are named and skipped)
        for p in sorted(Path(cfg["directory"]).iterdir()):
            if p.is_file() and p.suffix in (".npz", ".ply"):
                pipeline.process_cloud(p)
            elif p.is_file():
                print(f"skipping {p}: not a point cloud format this build reads (.npz / .ply)")
    else:
        print("Please supply a path or directory.")


if __name__ == "__main__":
    main()
