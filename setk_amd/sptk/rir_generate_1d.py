#!/usr/bin/env python
"""
Room impulse responses for simulated far-field data, linear arrays, on the MI355X.

Drop-in for funcwj/setk ``scripts/sptk/rir_generate_1d.py`` (same arguments, the same ``Room`` /
``RoomGenerator`` / ``RirSimulator`` behaviour, log lines, ``rir.json`` and room plots).  The
reference samples a room, an array position and the speakers with the module ``random`` and calls
``rir-simulate`` (src/rir-simulate.cc) once per speaker.  Its sampling makes no draw while a RIR is
generated, so this front end samples EVERY room, array and speaker first -- in the reference's draw
order, retries included -- and then hands the RIRs to ``engine.BatchRirGenerator`` in batches of
``--batch-rirs``: the image method runs on the device for the whole batch (setk_rir_generate_batch).

What reaches the generator is what ``Room.rir`` (:126-168) puts on the command line: every value
formatted ``"{:.3f}"``.  The RIRs are written with ``write_wav`` as the reference's pyrirgen branch
does (:183); see tests/PARITY_NOTES_RIR.md for the one LSB that may separate it from Kaldi's writer.

Options of this repository: ``--batch-rirs`` and ``--seed`` (the reference never seeds ``random``).
``--gpu true`` is refused: gpuRIR has its own Sabine estimate and file naming and is not available
to compare against.  The reference's ``_place_spk`` reads a module-global ``args`` (:276, :283); here
it reads the simulator's own.
"""
import argparse
import json
import random
from pathlib import Path

import numpy as np

from setk_amd import _ffi
from setk_amd.libs.opts import str2tuple, strtobool
from setk_amd.libs.rir import three_decimals
from setk_amd.libs.sampler import UniformSampler
from setk_amd.libs.utils import get_logger, write_wav

default_dpi = 200
default_fmt = "jpg"

GPU_REASON = ("--gpu true is not supported: gpuRIR computes its coefficients with its own Sabine estimate, names "
              "its files differently and is not available to compare against; the image method of rir-simulate "
              "runs on the device without it")

logger = get_logger(__name__)


class Room(object):
    """
    Room instance
    """

    def __init__(self, l, w, h, rt60=None, refl=None):  # noqa: E741
        self.size = (l, w, h)
        self.beta = rt60 if rt60 is not None else [refl] * 6
        self.memo = "{}={:.2f}".format("RT60" if rt60 is not None else "Refl", rt60 if rt60 is not None else refl)

    def set_mic(self, topo, center, vertical=False):
        """
        Place microphone array
        topo: tuple like (x1, x2, ...)
        center: center 3D postion for microphone array
        """
        Mx, My, Mz = center
        Mc = (topo[-1] - topo[0]) / 2
        if not vertical:
            self.rpos = [(Mx - Mc + x, My, Mz) for x in topo]
        else:
            self.rpos = [(Mx, My - Mc + x, Mz) for x in topo]
        self.topo = topo
        self.rcen = (Mx, My)

    def set_spk(self, pos):
        """
        Place sound source (speaker)
        """
        self.spos = pos

    def conf(self):
        """
        Return configure of room (exclude sound sources)
        """
        Rf = lambda f: round(f, 3)  # noqa: E731
        return {
            "beta": [Rf(f) for f in self.beta] if isinstance(self.beta, list) else Rf(self.beta),
            "receiver_location": [tuple(Rf(n) for n in p) for p in self.rpos],
            "room_size": [Rf(n) for n in self.size],
            "receiver_geometric": self.topo
        }

    def plot(self, scfg, dest, room_id):
        """
        Visualize microphone array and speakers in current room
        """
        import matplotlib.pyplot as plt
        plt.switch_backend("agg")
        fig, ax = plt.subplots()
        ax.set_aspect("equal", "box")
        # constraint length and width
        l, w, _ = self.size  # noqa: E741
        ax.set_xlim((0, l))
        ax.set_ylim((0, w))
        # draw microphone array
        ax.plot([p[0] for p in self.rpos], [p[1] for p in self.rpos], "k.")
        ax.plot([self.rcen[0]], [self.rcen[1]], "r+")
        # draw each speaker
        spkx = [cfg["pos"][0] for cfg in scfg]
        spky = [cfg["pos"][1] for cfg in scfg]
        ax.plot(spkx, spky, "k+")
        # labels and ticks
        ax.set_xlabel(f"Length ({l:.2f}m)")
        ax.set_xticks([round(x, 1) for x in np.linspace(0, l, 5)])
        ax.set_ylabel(f"Width ({w:.2f}m)")
        ax.set_yticks([round(y, 1) for y in np.linspace(0, w, 5)])
        ax.set_title(f"{room_id} ({self.memo})")
        fig.savefig(dest, dpi=default_dpi, format=default_fmt)
        plt.close(fig)

    def rir(self, sr=16000, rir_nsamps=4096, v=340):
        """
        The generator's arguments for the current settings: what the reference's rir-simulate
        command line carries (:151-168), every value through "{:.3f}"
        """
        beta = three_decimals(self.beta) if isinstance(self.beta, list) else round(self.beta, 3)
        return dict(room=three_decimals(self.size), src=three_decimals(self.spos),
                    mics=[three_decimals(p) for p in self.rpos], beta_or_rt60=beta, sr=sr, rir_nsamps=rir_nsamps,
                    v=v, hp_filter=True)


class RoomGenerator(object):
    """
    Room generator
    """

    def __init__(self, rt60_opt, absc_opt, room_dim):
        """
        rt60_opt: "" or "a,b", higher priority than absc_opt
        absc_opt: tuple like (a,b)
        room_dim: str like "a,b;c,d;e,d"
        """
        self.rt60_opt = rt60_opt
        if not rt60_opt:
            self.absc = UniformSampler(absc_opt)
        else:
            rt60_r = str2tuple(rt60_opt)
            self.rt60 = UniformSampler(rt60_r)
        dim_range = [str2tuple(t) for t in room_dim.split(";")]
        if len(dim_range) != 3:
            raise RuntimeError(f"Wrong format with --room-dim={room_dim}")
        self.dim_sampler = [UniformSampler(c) for c in dim_range]

    def generate(self, v=340):
        # (l, w, h)
        (l, w, h) = (s.sample() for s in self.dim_sampler)  # noqa: E741
        if self.rt60_opt:
            # no reflection is ok
            if self.rt60.max == 0:
                return Room(l, w, h, rt60=0)
            else:
                # check rt60 here
                S, V = l * w * h, (l * w + l * h + w * h) * 2
                # sabine formula
                rt60_min = 24 * V * np.log(10) / (v * S)
                if rt60_min >= self.rt60.max:
                    return None
                else:
                    rt60 = random.uniform(rt60_min, self.rt60.max)
                    return Room(l, w, h, rt60=rt60)
        else:
            absc = self.absc.sample()
            return Room(l, w, h, refl=np.sqrt(1 - absc))


class RirSimulator(object):
    """
    RIR simulator: run() samples every room first, then generates the RIRs in device batches
    """

    def __init__(self, args):
        if args.gpu:
            raise _ffi.SetkUnsupported(GPU_REASON)
        # make dump dir
        Path(args.dump_dir).mkdir(exist_ok=True, parents=True)
        self.rirs_cfg = []
        self.room_generator = RoomGenerator(args.rt60, args.abs_range, args.room_dim)
        self.mx, self.my = args.array_relx, args.array_rely
        self.vertical = getattr(args, "vertical", False)
        self.sr = args.sr
        self.args = args
        self.jobs = []    # (generator arguments, destination) in the reference's order of rir-simulate calls
        self.plots = []   # (room, speaker configurations, destination, title)

    def _place_mic(self, room):
        x, y, _ = room.size
        # sample array location
        # (mx, my) center postion of array
        mx = random.uniform(*(x * v for v in self.mx))
        my = random.uniform(*(y * v for v in self.my))
        mz = random.uniform(*self.args.array_height)
        # place array
        room.set_mic(self.args.array_topo, (mx, my, mz), vertical=self.vertical)
        return (mx, my), room

    def _max_src_dist(self, rpos_2d, room_size_2d):
        mx, my = rpos_2d
        rx, ry = room_size_2d
        bound = [(0, 0), (0, ry), (rx, 0), (rx, ry)]
        dist = [((mx - x)**2 + (my - y)**2)**0.5 for (x, y) in bound]
        return max(dist)

    def _sample_doa(self):
        # sample from 0-180
        return random.uniform(0, np.pi)

    def _place_spk(self, center, room):
        args = self.args
        num_rirs = args.num_rirs
        done, ntry = 0, 0
        mx, my = center
        rx, ry, rz = room.size
        max_retry = args.retry * num_rirs
        stats = []

        min_src_dist, max_src_dist = args.src_dist
        max_src_dist = min(max_src_dist, self._max_src_dist((mx, my), (rx, ry)))
        Rf = lambda f: round(f, 3)  # noqa: E731
        while True:
            ntry += 1
            if ntry > max_retry:
                break
            sz = random.uniform(*args.speaker_height)
            if sz >= rz:
                continue
            # speaker distance
            dst = random.uniform(min_src_dist, max_src_dist)
            doa = self._sample_doa()
            if not self.vertical:
                sx = mx + np.cos(doa) * dst
                sy = my + np.sin(doa) * dst
            else:
                sx = my - np.cos(doa) * dst
                sy = mx + np.sin(doa) * dst
            # check speaker location
            if 0 >= sx or sx >= rx or 0 >= sy or sy >= ry:
                continue
            done += 1
            stat = {"pos": (Rf(sx), Rf(sy), Rf(sz)), "doa": Rf(doa * 180 / np.pi), "dst": Rf(dst)}
            stats.append(stat)
            if done == num_rirs:
                break
        logger.info(f"Put speaker point: try/done = {ntry}/{done}")
        return done == num_rirs, stats

    def run_for_instance(self, room_id):
        room = None
        while not room:
            room = self.room_generator.generate(v=self.args.speed)
        rpos, room = self._place_mic(room)
        succ, scfg = self._place_spk(rpos, room)
        if succ:
            rcfg = room.conf()
            for idx, cfg in enumerate(scfg):
                cfg["loc"] = f"{self.args.dump_dir}/Room{room_id}-{idx + 1}.wav"
            for cfg in scfg:
                # place spk; its rir is generated with the batch
                room.set_spk(cfg["pos"])
                self.jobs.append((room.rir(sr=self.sr, rir_nsamps=int(self.sr * self.args.rir_dur), v=self.args.speed),
                                  cfg["loc"]))
            self.plots.append((room, scfg, f"{self.args.dump_dir}/Room{room_id}.{default_fmt}", f"Room{room_id}"))
            rcfg["spk"] = scfg
            self.rirs_cfg.append(rcfg)
        return succ

    def generate(self):
        """The sampled RIRs in batches of --batch-rirs, each written where the reference writes it."""
        _ffi.set_torch_free()  # the engine brings its own buffers and stream
        from setk_amd.engine import BatchRirGenerator
        engine = BatchRirGenerator()
        step = max(1, self.args.batch_rirs)
        try:
            for b in range(0, len(self.jobs), step):
                batch = self.jobs[b:b + step]
                rirs = engine.run([spec for spec, _ in batch])
                for (_, loc), rir, status in zip(batch, rirs, engine.status):
                    if status != _ffi.NUM_OK:
                        raise RuntimeError(f"{loc}: NaN / inf in the settings or a speaker on a microphone "
                                           f"(status {status}), no RIR")
                    write_wav(loc, rir, sr=self.sr)
        finally:
            engine.close()
        for room, scfg, dest, title in self.plots:
            room.plot(scfg, dest, title)

    def run(self):
        num_rooms = self.args.num_rooms
        max_retry = self.args.retry * num_rooms
        done, ntry = 0, 0
        while True:
            ntry += 1
            if ntry > max_retry:
                break
            succ = self.run_for_instance(done + 1)
            if succ:
                done += 1
            if done == num_rooms:
                break
        self.generate()
        # dump rir configurations
        with open(Path(self.args.dump_dir) / "rir.json", "w") as f:
            json.dump(self.rirs_cfg, f, indent=2)
        logger.info(f"Generate {self.args.num_rirs * num_rooms:d} rirs, " + f"{done:d} rooms done, try = {ntry}")


def run(args, simulator=RirSimulator):
    if args.seed is not None:
        random.seed(args.seed)
    simulator(args).run()


def build_parser(two_d=False):
    parser = argparse.ArgumentParser(
        description="Command to generate single/multi-channel RIRs "
        "(the image method of rir-simulate, on the device). "
        "In this command, we will simulate several rirs for each room, which is "
        "configured using --num-rirs",
        formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    parser.add_argument("num_rooms", type=int, help="Total number of rooms to simulate")
    parser.add_argument("--num-rirs", type=int, default=40, help="Number of rirs to simulate for each room")
    parser.add_argument("--dump-cfg", type=strtobool, default=True,
                        help="If true, dump rir configures out in json format")
    parser.add_argument("--rir-dur", type=float, default=0.5, help="Duration of the simulated rir (s)")
    parser.add_argument("--sr", type=int, default=16000, help="Sample rate of simulated signal")
    parser.add_argument("--dump-dir", type=str, default="rir", help="Directory to dump generated rirs")
    parser.add_argument("--room-dim", type=str, default="7,10;7,10;3,4",
                        help="Constraint for room length/width/height, separated by semicolon")
    if not two_d:
        parser.add_argument("--vertical-oriented", type=strtobool, dest="vertical", default=False,
                            help="Orientation to place microphone array (vertical or horizontal)")
    parser.add_argument("--array-height", type=str2tuple, default=(1, 2), help="Range of array's height")
    parser.add_argument("--array-relx", type=str2tuple, default=(0.4, 0.6),
                        help="Area of room to place microphone array randomly"
                        "(relative values to room's length)")
    parser.add_argument("--array-rely", type=str2tuple, default=(0.4, 0.6) if two_d else (0.05, 0.1),
                        help="Area of room to place microphone array randomly"
                        "(relative values to room's width)")
    parser.add_argument("--speaker-height", type=str2tuple, default=(1.6, 2), help="Range of speaker's height")
    if two_d:
        parser.add_argument("--array-topo", type=str, default="0,0.05;0.05,0;0,-0.05;-0.05,0",
                            help="Topology of the 2D microphone arrays.")
    else:
        parser.add_argument("--array-topo", type=str2tuple, default=(0, 0.1, 0.2, 0.3),
                            help="Linear topology for microphone arrays.")
    parser.add_argument("--absorption-coefficient-range", type=str2tuple, dest="abs_range", default=(0.2, 0.8),
                        help="Range of absorption coefficient "
                        "of the room material. Absorption coefficient "
                        "is located between 0 and 1, if a material "
                        "offers no reflection, the absorption "
                        "coefficient is close to 1.")
    parser.add_argument("--rt60", type=str, default="0.2,0.7",
                        help="Range of RT60, this option has higher priority than "
                        "--absorption-coefficient-range")
    parser.add_argument("--sound-speed", type=float, dest="speed", default=343 if two_d else 340,
                        help="Speed of sound")
    parser.add_argument("--retry", type=int, default=5,
                        help="Max number of times tried to generate rirs "
                        "for a specific room (retry * num_rirs)")
    parser.add_argument("--source-distance", type=str2tuple, dest="src_dist", default=(1, 3) if two_d else (1.5, 3),
                        help="Range of distance between microphone arrays and speakers")
    parser.add_argument("--gpu", type=strtobool, default=False,
                        help="Refused: gpuRIR (https://github.com/DavidDiazGuerra/gpuRIR.git) is not ported")
    parser.add_argument("--batch-rirs", type=int, default=64, help="[setk_amd] RIRs per batched call")
    parser.add_argument("--seed", type=int, default=None,
                        help="[setk_amd] seed of the module random (the reference never seeds it)")
    return parser


def main(argv=None):
    run(build_parser().parse_args(argv))


if __name__ == "__main__":
    main()
