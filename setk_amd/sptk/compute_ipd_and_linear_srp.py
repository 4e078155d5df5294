#!/usr/bin/env python
"""
Typical spatial features (SRP / IPD) on the MI355X.

Drop-in for funcwj/setk ``scripts/sptk/compute_ipd_and_linear_srp.py`` (same positional
arguments, options, defaults and Kaldi archive output).  Where the reference walks a
SpectrogramReader one utterance at a time through numpy, this front end feeds batches of WAVE
SAMPLES to ``engine.BatchSpatialFeatures``: one upload per batch, the spectrograms stay on the
device (setk_stft_batch -> setk_spatial_batch), one download of the feature maps.
``--type msc`` is refused: see setk_amd.libs.spatial.MSC_REASON.
Under ``torchrun`` every rank would write the same archive, so the tool runs on one rank only.
"""
import argparse

from setk_amd import _ffi
from setk_amd.engine import BatchSpatialFeatures
from setk_amd.libs.data_handler import ArchiveWriter, WaveReader
from setk_amd.libs.opts import StftParser, str2tuple, strtobool
from setk_amd.libs.spatial import MSC_REASON
from setk_amd.libs.utils import get_logger
from setk_amd.sptk._common import read_samples, run_batches, stft_kwargs

logger = get_logger(__name__)


def feed(engine, waves, keys, batch_utts, on_result, doa_index=None):
    """Read the utterances `keys` of the wave table, run them through the engine in batches of
    batch_utts and hand (key, features) to on_result in the table's order."""
    def flush(queue):
        idx = [doa_index[k] for k, _ in queue] if doa_index is not None else None
        for (key, _), feats in zip(queue, engine.run([s for _, s in queue], doa_index=idx)):
            on_result(key, feats)
        return len(queue)

    run_batches(((key, read_samples(waves, key)) for key in keys), batch_utts, flush)


def parse_ipd_pairs(text):
    pairs = []
    for p in text.split(";"):
        indexes = list(map(int, p.split(",")))
        if len(indexes) != 2:
            raise ValueError("Invalid --ipd.pair configuration " + f"detected: {text}")
        pairs.append(tuple(indexes))
    return pairs


def build_engine(args):
    if args.type == "srp":
        return BatchSpatialFeatures("srp_linear", topo=tuple(args.linear_topo), num_doa=args.num_doa,
                                    samp_tdoa=bool(args.samp_tdoa), sample_rate=args.samp_frequency,
                                    **stft_kwargs(args))
    if args.type == "ipd":
        return BatchSpatialFeatures("ipd", pairs=parse_ipd_pairs(args.ipd_pair), cos=bool(args.ipd_cos),
                                    sin=bool(args.ipd_sin), **stft_kwargs(args))
    raise _ffi.SetkUnsupported(MSC_REASON)


def run(args):
    engine = build_engine(args)
    waves = WaveReader(args.wav_scp)
    # device buffers, streams and copies come from the library unless a table is wider than the
    # fused STFT (more than 8 channels go through torch tensors)
    _ffi.set_torch_free(waves.first_channels_at_most(8))
    num_utts = 0
    with ArchiveWriter(args.dup_ark, args.scp) as writer:

        def on_result(key, feats):
            nonlocal num_utts
            writer.write(key, feats)
            num_utts += 1
            if not num_utts % 1000:
                logger.info(f"Processed {num_utts} utterance...")

        feed(engine, waves, waves.index_keys, args.batch_utts, on_result)
    engine.close()
    logger.info(f"Processed {args.type.upper()} for {num_utts} utterances")


def build_parser():
    parser = argparse.ArgumentParser(
        description="Command to compute some typical spatial features, egs: SRP/MSC/IPD. ("
        "SRP: SRP-PHAT Anguler Spectrum, MSC: Magnitude Squared Coherence, "
        "IPD: Interchannel Phase Difference)",
        formatter_class=argparse.ArgumentDefaultsHelpFormatter, parents=[StftParser.parser])
    parser.add_argument("wav_scp", type=str, help="Multi-Channel wave scripts in kaldi format")
    parser.add_argument("dup_ark", type=str, help="Location to dump features in kaldi's archives")
    parser.add_argument("--scp", type=str, default="",
                        help="If assigned, generate corresponding feature scripts")
    parser.add_argument("--type", type=str, default="srp", choices=["srp", "msc", "ipd"],
                        help="Type of spatial features to compute")
    parser.add_argument("--srp.sample-rate", type=int, dest="samp_frequency", default=16000,
                        help="Sample frequency of input wave")
    parser.add_argument("--srp.sample-tdoa", type=strtobool, default=False, dest="samp_tdoa",
                        help="Sample TDoA instead of DoA when computing spectrum")
    parser.add_argument("--srp.num_doa", type=int, dest="num_doa", default=181,
                        help="Number of DoA to sampled from 0 to 180 degress")
    parser.add_argument("--srp.topo", type=str2tuple, dest="linear_topo", default="0,0.2,0.4,0.8",
                        help="Topology description of microphone arrays")
    parser.add_argument("--ipd.cos", dest="ipd_cos", type=strtobool, default=False,
                        help="Compute cosIPD instead of IPD")
    parser.add_argument("--ipd.sin", dest="ipd_sin", type=strtobool, default=False,
                        help="Append sinIPD to cosIPD spatial features")
    parser.add_argument("--ipd.pair", type=str, dest="ipd_pair", default="0,1",
                        help="Given several channel index pairs to compute IPD spatial features, "
                        "separated by semicolon, egs: 0,3;1,4")
    parser.add_argument("--msc.ctx", type=int, dest="msc_ctx", default=1,
                        help="Value of context in MSC computation (MSC is not ported)")
    parser.add_argument("--batch-utts", type=int, default=32, help="[setk_amd] utterances per GPU batch")
    return parser


def main(argv=None):
    run(build_parser().parse_args(argv))


if __name__ == "__main__":
    main()
