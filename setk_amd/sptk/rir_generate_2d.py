#!/usr/bin/env python
"""
Room impulse responses for simulated far-field data, planar (2D) arrays, on the MI355X.

Drop-in for funcwj/setk ``scripts/sptk/rir_generate_2d.py``: ``rir_generate_1d.py`` with the array
given as "x1,y1;x2,y2;..." around its centre (:65-74), no orientation switch, speakers sampled over
the full circle (:286-291) and its own defaults (array-rely, sound-speed 343, source-distance).
Everything else -- sampling first, device batches, ``--batch-rirs``, ``--seed``, the refused
``--gpu`` -- is rir_generate_1d.py's.
"""
import random

import numpy as np

from setk_amd.libs.opts import str2tuple
from setk_amd.sptk import rir_generate_1d as one_d


class Room(one_d.Room):

    def set_mic(self, topo, center, vertical=False):
        """
        Place microphone array
        topo: tuple like [(x1, y1), ...]
        center: center 3D postion for microphone array
        """
        Mx, My, Mz = center
        self.rpos = [(Mx + x, My + y, Mz) for (x, y) in topo]
        self.topo = topo
        self.rcen = (Mx, My)


class RoomGenerator(one_d.RoomGenerator):

    def generate(self, v=340):
        room = super().generate(v=v)
        if room is not None:
            room.__class__ = Room
        return room


class RirSimulator(one_d.RirSimulator):

    def __init__(self, args):
        super().__init__(args)
        self.room_generator = RoomGenerator(args.rt60, args.abs_range, args.room_dim)
        self.array_topo = [str2tuple(t) for t in args.array_topo.split(";")]

    def _place_mic(self, room):
        x, y, _ = room.size
        mx = random.uniform(*(x * v for v in self.mx))
        my = random.uniform(*(y * v for v in self.my))
        mz = random.uniform(*self.args.array_height)
        room.set_mic(self.array_topo, (mx, my, mz))
        return (mx, my), room

    def _sample_doa(self):
        # sample from 0-360
        return random.uniform(0, np.pi * 2)


def build_parser():
    return one_d.build_parser(two_d=True)


def main(argv=None):
    one_d.run(build_parser().parse_args(argv), simulator=RirSimulator)


if __name__ == "__main__":
    main()
