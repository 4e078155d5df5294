#!/usr/bin/env python
"""
Compute steer vectors (based on array geometry) for linear / circular arrays.

Drop-in for funcwj/setk ``scripts/sptk/compute_steer_vector.py`` (same positional argument,
options and defaults, :54-105): the A x M x F complex array that ``do_ssl.py`` reads, saved with
``np.save``.  Host only, on ``libs.beamformer.linear_steer_vector`` / ``circular_steer_vector``.
"""
import argparse

import numpy as np

from setk_amd.libs.beamformer import circular_steer_vector, linear_steer_vector
from setk_amd.libs.opts import str2tuple, strtobool


def steer_vectors(args):
    """A x M x F (compute_steer_vector.py:17-50)."""
    if args.geometry == "linear":
        topo = np.array(args.linear_topo)
        sv = [linear_steer_vector(topo, doa, args.num_bins, c=args.speed, sr=args.sr)
              for doa in np.linspace(0, 180, args.num_doas)]
    else:
        sv = [circular_steer_vector(args.circular_radius, args.circular_around, doa, args.num_bins,
                                    c=args.speed, sr=args.sr, center=args.circular_center)
              for doa in np.arange(0, 360, 360 / args.num_doas)]
    sv = np.stack(sv)  # A x F x M
    if args.normalize:
        sv = sv / sv.shape[-1]**0.5
    return sv.transpose(0, 2, 1)


def run(args):
    np.save(args.steer_vector, steer_vectors(args))


def build_parser():
    parser = argparse.ArgumentParser(
        description="Command to compute steer vectors, using for SSL & BF & AF computation",
        formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    parser.add_argument("steer_vector", type=str, help="Output location of the steer vector")
    parser.add_argument("--num-doas", type=int, default=181, help="Step size when sampling the DoA")
    parser.add_argument("--num-bins", type=int, default=257, help="Number of the FFT points used")
    parser.add_argument("--sr", type=int, default=16000, help="Sample rate of input wave")
    parser.add_argument("--speed", type=float, default=343, help="Speed of sound")
    parser.add_argument("--linear-topo", type=str2tuple, default=(),
                        help="Topology of linear microphone arrays")
    parser.add_argument("--circular-around", type=int, default=6,
                        help="Number of the micriphones in circular arrays")
    parser.add_argument("--circular-radius", type=float, default=0.05, help="Radius of circular array")
    parser.add_argument("--circular-center", type=strtobool, default=False,
                        help="Is there a microphone put in the center of the circular array?")
    parser.add_argument("--geometry", type=str, choices=["linear", "circular"], default="linear",
                        help="Geometry of the microphone array")
    parser.add_argument("--normalize", type=strtobool, default=False,
                        help="Normalzed steer vector or not")
    return parser


def main(argv=None):
    run(build_parser().parse_args(argv))


if __name__ == "__main__":
    main()
