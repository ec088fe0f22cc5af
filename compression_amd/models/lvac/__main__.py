"""`python -m compression_amd.models.lvac train|test|reconstruct`, one flag per Config field."""
import argparse
import dataclasses
import os
import sys

import numpy as np

from .model import Config, convert_yuv_to_rgb, main
from .ply import create_new_plyfile


def _flag_type(field):
    if field.type in (bool, "bool"):
        return lambda s: s.lower() in ("1", "true", "yes", "on")
    return {"int": int, "float": float, "str": str}.get(field.type, field.type)


def parse_args(argv):
    parser = argparse.ArgumentParser(prog="python -m compression_amd.models.lvac", description=__doc__)
    parser.add_argument("command", choices=("train", "test", "reconstruct"))
    for field in dataclasses.fields(Config):
        parser.add_argument("--" + field.name, type=_flag_type(field), default=field.default)
    parser.add_argument("--device", default=None, help="torch device; a HIP device if there is one")
    parser.add_argument("--output", default=None, help="reconstruct: the PLY file to write")
    args = parser.parse_args(argv)
    config = Config(**{f.name: getattr(args, f.name) for f in dataclasses.fields(Config)})
    return args, config


def reconstruct(config, device=None, output=None):
    """Decodes the colours from the newest checkpoint and writes a copy of the original PLY that carries them."""
    colours = main(config, training=False, return_attributes=True, device=device)
    extractor = config.extractor_model
    if config.distortion_colorspace.lower() == "yuv":
        colours = convert_yuv_to_rgb(colours)
    if output is None:
        base, ext = os.path.splitext(config.original_vpc)
        output = f"{base}_lambda{config.entropy_multiplier}_{extractor}{ext}"
    create_new_plyfile(config.original_vpc, output, np.asarray(colours.detach().cpu()))
    return output


def run(argv=None):
    args, config = parse_args(sys.argv[1:] if argv is None else argv)
    if args.command == "train":
        main(config, training=True, device=args.device)
    elif args.command == "test":
        main(config, training=False, device=args.device)
    else:
        print("Wrote", reconstruct(config, args.device, args.output))


if __name__ == "__main__":
    run()
