"""Command line: WAV files -> MIDI files (the notebook's upload / transcribe / download cells in one call).

    python -m mt3_amd.transcribe --checkpoint PATH [--model mt3|ismir2021] [--dtype float32|bfloat16]
                                 [--decoding beam1|greedy|beam|sample] [--num-beams K] [--confidences]
                                 [--temperature T] [--top-k K] [--top-p P] [--seed N]
                                 [--programs P[,P...]] [--no-drums] [--pianoroll [FPS]] [--render [RATE]]
                                 [--score-against DIR] [--score-midi DIR [--score-shifts S,...]]
                                 [--align-midi DIR [--align-max-shift S] [--align-step S] [--align-smoothness L]]
                                 [--sync-midi DIR [--sync-pool P]]
                                 [--consensus N [--consensus-min-votes M] [--consensus-tolerance S]]
                                 [--sustain] [--trim-overlaps]
                                 [--velocities [--velocity-gamma G] [--velocity-anchor V]]
                                 [--beats [--beats-prior-bpm B] [--quantize SUBDIV]]
                                 [--harmony [--harmony-change-penalty P]]
                                 IN.wav [IN2.wav ...] [-o OUT]

Writes IN.mid beside each input, or to OUT: a file for one input, a directory for several.  All inputs go through the
engine as one job (`InferenceModel.transcribe_wavs`).  --checkpoint is handed to `InferenceModel` as it is: a t5x
checkpoint directory, a flat or compact `.npz`, or `random:<seed>`.  --decoding beam runs t5x beam_search with
--num-beams K decodes (1 .. 8) per segment (`InferenceModel(decoding="beam", num_beams=K)`).  --confidences also writes
NAME.confidence.json beside each NAME.mid: one record per note, in the NoteSequence's order, with the note's fields and
`onset_logprob`, `end_logprob` (null where no token ended the note) and `onset_margin` of
`InferenceModel.transcribe_wav_scored` (each file is then a job of its own: decode, then one scoring pass).
--programs 0,33 restricts the decode of every input to those MIDI programs and --no-drums forbids drum notes (constrained
decoding: the excluded tokens cannot be picked; `InferenceModel(..., programs=, drums=)`).
--decoding sample draws every token from softmax(logits / T) (t5x temperature_sample), cut to the --top-k most likely
tokens or to the smallest set of probability --top-p; --seed picks the draw, which for a file is the same whatever other
inputs share the job (`InferenceModel(decoding="sample", temperature=, top_k=, top_p=, seed=)`).
--pianoroll [FPS] also writes NAME.npy beside each NAME.mid: the transcription's piano roll, uint16 [128, frames] at FPS
frames per second (default 62.5), each note's velocity summed into its frames (cut at 65535), drum notes silent
(`mt3_amd.pianoroll.pianorolls`: the rolls of all inputs are rasterised in one call once the job's notes are decoded).
--render [RATE] also writes NAME.render.wav beside each NAME.mid: the transcription as mono int16 audio at RATE Hz (default
16000), peak 0.9, to listen to (`mt3_amd.render.render`: one timbre for every program, a noise burst per drum note; all
inputs are rendered in one call).  It is the sound of the notes as NAME.mid holds them, times on the file's tick grid.
--score-against DIR scores the job: for each input NAME.wav it reads DIR/NAME.mid as the reference, runs
`metrics.transcription_metrics` on all (reference, transcription) pairs once -- every note matching of the job in one
device call -- and writes scores.json into the output directory: {"files": {NAME: {key: value}}, "mean": {key: value}}.
The output directory is the one the MIDI files go to; inputs that would be written to several directories (no -o, inputs
in different places) are refused with --score-against: give -o DIR.
--align-midi DIR repairs the timing of known notes: for each input NAME.wav it reads DIR/NAME.mid, finds a time shift per
segment of the audio (`InferenceModel.align_notes_many`: all inputs as one job; shifts of -S .. S seconds from
--align-max-shift, default 0.2, in steps of --align-step, default 0.02; --align-smoothness: log-probability per second
of jump between neighbouring segments) and writes the moved notes as NAME.aligned.mid beside NAME.mid, and one
alignment.json into the output directory: a list with one record per input, in input order -- "audio", "segment_shifts",
"path_score", "flat_shift", "flat_score" (same one-directory rule as --score-against).
--sync-midi DIR synchronises a score to each recording: for each input NAME.wav it reads DIR/NAME.mid (a score: quantised,
another tempo), finds the dynamic-time-warping path between the chroma of the audio and of the notes
(`InferenceModel.synchronize_many`: all inputs as one job on the device, no decode of its own; --sync-pool P log-mel frames
per feature frame, 1 .. 16, default 5) and writes the notes in the recording's time as NAME.synced.mid beside NAME.mid, and
one sync.json into the output directory: a list with one record per input, in input order -- "audio", "total",
"mean_cost", "tempo_ratio" and "path", [audio seconds, score seconds] pairs thinned to one per second of audio (same
one-directory rule as --score-against).  It goes with every other flag: the transcription is written as without it.
--consensus N writes as NAME.mid the notes that N sampled transcriptions of the input agree on
(`InferenceModel.consensus_many`: N draws with the sampling parameters of --temperature / --top-k / --top-p and seeds
--seed .. --seed + N - 1, all input files and all their draws as ONE engine job in which every segment is encoded once,
voted on the device; a note is kept when --consensus-min-votes of them have it, default a strict majority; onsets within
--consensus-tolerance seconds, default 0.05, are one note), and NAME.votes.json beside it:
{"n_voters": N, "min_votes": M, "notes": [...]}, one record per note of NAME.mid in the NoteSequence's order with its
start_time, end_time, pitch, program, is_drum, votes and members.  (--well-formed-tied keeps N decodes per job.)  Not with
--decoding beam, and not together with --confidences.
--sustain and --trim-overlaps prepare the MIDI files read for --score-against, --score-midi, --align-midi and --sync-midi the way the
reference prepares its targets (`mt3_amd.note_prep.prepare`, on the device, all files of an option as one job): --sustain
applies each file's sustain pedal (controller 64) to its notes' ends -- what a piano model such as ismir2021 was trained
on; --trim-overlaps then trims overlapping notes of one pitch and program and drops the empty ones.
--velocities gives every note a velocity estimated from the log-mel the decode has just read (`InferenceModel(...,
velocities=)`, `mt3_amd.velocity.estimate`: the note's level at its onset against the file's median note, which gets
--velocity-anchor, default 80; amplitude ~ (velocity / 127)^G with --velocity-gamma G, default 2.0) before NAME.mid,
--render and --pianoroll are written; the mt3 model alone gives every note the same velocity, 127.  With --consensus or
--confidences the estimate runs on the finished notes (`InferenceModel.note_velocities_many`).  Not with --model ismir2021.
--beats finds the beats of every input from its transcription's own onsets (`mt3_amd.beats.track`: all inputs as one job
on the device; one tempo per file, found under a prior centred on --beats-prior-bpm, default 120) and writes NAME.mid
with the tempo map -- a set-tempo event on every beat, every beat one quarter note, so the file plays as performed and
opens on the grid of a notation editor -- and NAME.beats.json beside it: {"qpm", "period_frames", "beats": [seconds]}.
An input in which no beat is found keeps the constant 120 qpm.  --quantize SUBDIV first moves the notes onto the grid of
SUBDIV steps per beat (1 .. 48; `mt3_amd.beats.snap`), before NAME.mid, --render and --pianoroll are written.
--harmony (it implies --beats) finds each input's key, the chord of every beat, the bar length and the downbeats from its
notes and beats (`mt3_amd.harmony.analyze`: all inputs as one job on the device; --harmony-change-penalty P, 0 .. 2^20,
default 857: what the chord path pays for a change) and writes NAME.mid with a key signature, a time signature and a marker
per chord change in the tempo map's track, tick 0 on a downbeat, and NAME.harmony.json beside it: {"key", "key_name",
"sharps", "beats_per_bar", "downbeat", "downbeats": [seconds], "chords": [[start, end, name]]}.  With --quantize the
analysis reads the notes as they are written, on the grid.
"""
from __future__ import annotations

import argparse
import json
import math
import os
import sys


def plan(argv=None):
    """parse the arguments and decide every output path; nothing is loaded or built.  Exits (status 2, message on
    stderr) on a missing input or an -o that cannot hold the outputs."""
    ap = argparse.ArgumentParser(prog="python -m mt3_amd.transcribe", description="Transcribe WAV files to MIDI.")
    ap.add_argument("--checkpoint", required=True, help="t5x checkpoint directory, .npz, or random:<seed>")
    ap.add_argument("--model", default="mt3", choices=("mt3", "ismir2021"))
    ap.add_argument("--dtype", default="float32", choices=("float32", "bfloat16"))
    ap.add_argument("--temperature", type=float, default=1.0, metavar="T", help="--decoding sample: the temperature (> 0)")
    ap.add_argument("--top-k", type=int, default=0, metavar="K", help="--decoding sample: keep the K most likely tokens "
                    "(1 .. 256; 0: off)")
    ap.add_argument("--top-p", type=float, default=0.0, metavar="P", help="--decoding sample: keep the smallest set of "
                    "tokens of probability P (0 < P < 1; 0: off; not with --top-k)")
    ap.add_argument("--seed", type=int, default=0, metavar="N", help="--decoding sample: the seed of the draw")
    ap.add_argument("--decoding", default="beam1", choices=("beam1", "greedy", "beam", "sample"),
                    help="token selection: beam1 (default, the reference's), greedy, or beam (k-beam search, see --num-beams)")
    ap.add_argument("--num-beams", type=int, default=4, metavar="K", help="decodes per segment with --decoding beam (1 .. 8)")
    ap.add_argument("--confidences", action="store_true",
                    help="also write NAME.confidence.json beside each NAME.mid: per-note token log-probabilities")
    ap.add_argument("--programs", type=_program_list, default=None, metavar="P[,P...]",
                    help="constrained decoding: the MIDI programs (0 .. 127) the transcription may use, for all inputs")
    ap.add_argument("--no-drums", dest="drums", action="store_false", help="constrained decoding: no drum notes")
    ap.add_argument("--well-formed", action="store_true",
                    help="well-formed decoding: the token pick follows the event grammar (no backwards or repeated shift, "
                         "no stray tie), so nothing it emits is thrown away by the note decoder")
    ap.add_argument("--well-formed-notes", action="store_true",
                    help="note-consistent decoding: --well-formed plus the set of sounding notes, so no note-off of a silent "
                         "pitch, no pair tied twice and no drum at velocity 0 is emitted (models with a tie section)")
    ap.add_argument("--well-formed-tied", action="store_true",
                    help="tied decoding: --well-formed-notes, and every segment's tie section is forced to the notes the "
                         "file's previous segment left sounding; the inputs' segments are decoded in order, all files' "
                         "segment j together")
    ap.add_argument("--pianoroll", type=float, nargs="?", const=62.5, default=None, metavar="FPS",
                    help="also write NAME.npy beside each NAME.mid: the piano roll, uint16 [128, frames] at FPS frames "
                         "per second (default 62.5)")
    ap.add_argument("--render", type=int, nargs="?", const=16000, default=None, metavar="RATE",
                    help="also write NAME.render.wav beside each NAME.mid: the transcription as int16 audio at RATE Hz "
                         "(default 16000)")
    ap.add_argument("--score-against", default=None, metavar="DIR",
                    help="also write scores.json into the output directory: the transcription metrics of every input "
                         "NAME.wav against the reference DIR/NAME.mid, and their means (all MIDI files must go to one "
                         "directory: -o DIR for inputs in several)")
    ap.add_argument("--score-midi", default=None, metavar="DIR",
                    help="also write midi_scores.json into the output directory: how well the known notes DIR/NAME.mid "
                         "explain every input NAME.wav -- the model's teacher-forced loss on the MIDI's target tokens "
                         "(same one-directory rule as --score-against)")
    ap.add_argument("--score-shifts", type=_shift_list, default=None, metavar="S[,S...]",
                    help="--score-midi: also score the MIDI moved by each of these offsets in seconds, and report the best "
                         "(a list that starts with a minus sign is written --score-shifts=-0.1,0,0.1)")
    ap.add_argument("--align-midi", default=None, metavar="DIR",
                    help="also write NAME.aligned.mid beside each NAME.mid and alignment.json into the output directory: "
                         "the known notes DIR/NAME.mid moved by a time shift per segment so that they explain NAME.wav "
                         "best (same one-directory rule as --score-against)")
    ap.add_argument("--align-max-shift", type=float, default=None, metavar="S",
                    help="--align-midi: shifts of -S .. S seconds are tried (default 0.2)")
    ap.add_argument("--align-step", type=float, default=None, metavar="S", help="--align-midi: the step of the shifts "
                    "in seconds (default 0.02)")
    ap.add_argument("--align-smoothness", type=float, default=None, metavar="L",
                    help="--align-midi: log-probability a path pays per second of jump between neighbouring segments")
    ap.add_argument("--sync-midi", default=None, metavar="DIR",
                    help="also write NAME.synced.mid beside each NAME.mid and sync.json into the output directory: the "
                         "score DIR/NAME.mid moved onto the time of NAME.wav by dynamic time warping of chroma features "
                         "(same one-directory rule as --score-against)")
    ap.add_argument("--sync-pool", type=int, default=None, metavar="P",
                    help="--sync-midi: log-mel frames (8 ms) per feature frame, 1 .. 16 (default 5)")
    ap.add_argument("--consensus", type=int, default=None, metavar="N",
                    help="write the notes N sampled transcriptions agree on (1 .. 64) as NAME.mid, and NAME.votes.json "
                         "beside it: every note's votes and members")
    ap.add_argument("--consensus-min-votes", type=int, default=None, metavar="M",
                    help="--consensus: the samples that must have a note for it to be kept (1 .. N; default N // 2 + 1)")
    ap.add_argument("--consensus-tolerance", type=float, default=None, metavar="S",
                    help="--consensus: seconds between neighbouring onsets of one note's cluster (default 0.05)")
    ap.add_argument("--sustain", action="store_true",
                    help="--score-against / --score-midi / --align-midi: apply the sustain pedal (controller 64) of each "
                         "MIDI file read to its notes' ends")
    ap.add_argument("--trim-overlaps", action="store_true",
                    help="--score-against / --score-midi / --align-midi: trim overlapping notes of one pitch and program "
                         "in each MIDI file read, and drop the empty ones")
    ap.add_argument("--velocities", action="store_true",
                    help="estimate every note's velocity from the log-mel at its onset, relative to the file's median note "
                         "(the mt3 model gives every note the same velocity); applied before NAME.mid, --render and --pianoroll "
                         "are written")
    ap.add_argument("--velocity-gamma", type=float, default=None, metavar="G",
                    help="--velocities: amplitude ~ (velocity / 127)^G (default 2.0; 1.0 is what --render plays)")
    ap.add_argument("--velocity-anchor", type=float, default=None, metavar="V",
                    help="--velocities: the velocity of the file's median note (default 80)")
    ap.add_argument("--beats", action="store_true",
                    help="find each input's beats from its notes and write NAME.mid with the tempo map (every beat a quarter "
                         "note), and NAME.beats.json beside it")
    ap.add_argument("--beats-prior-bpm", type=float, default=None, metavar="B",
                    help="--beats: the centre of the tempo prior in beats per minute (default 120)")
    ap.add_argument("--quantize", type=int, default=None, metavar="SUBDIV",
                    help="--beats: move the notes onto the grid of SUBDIV steps per beat (1 .. 48) first")
    ap.add_argument("--harmony", action="store_true",
                    help="find each input's key, chords, bar length and downbeats (implies --beats) and write NAME.mid with "
                         "the key and time signatures and chord markers, and NAME.harmony.json beside it")
    ap.add_argument("--harmony-change-penalty", type=int, default=None, metavar="P",
                    help="--harmony: what the chord path pays for a change of chord, 0 .. 1048576 (default 857)")
    ap.add_argument("-o", "--output", help="output file (one input) or directory (several)")
    ap.add_argument("inputs", nargs="+", metavar="IN.wav")
    args = ap.parse_args(argv)
    if args.well_formed_notes:
        args.well_formed = "notes"
    if args.well_formed_tied:
        args.well_formed = "tied"
    if not 1 <= args.num_beams <= 8:
        ap.error("--num-beams must be 1 .. 8")
    if args.pianoroll is not None and not (math.isfinite(args.pianoroll) and args.pianoroll > 0):
        ap.error("--pianoroll takes a positive number of frames per second")
    if args.render is not None and not 1 <= args.render <= 384000:
        ap.error("--render takes a sample rate of 1 .. 384000 Hz")
    if args.consensus is None:
        for name in ("consensus_min_votes", "consensus_tolerance"):
            if getattr(args, name) is not None:
                ap.error("--%s needs --consensus" % name.replace("_", "-"))
    else:
        if not 1 <= args.consensus <= 64:
            ap.error("--consensus takes 1 .. 64 samples")
        if args.consensus_min_votes is not None and not 1 <= args.consensus_min_votes <= args.consensus:
            ap.error("--consensus-min-votes must be 1 .. %d (--consensus)" % args.consensus)
        if args.consensus_tolerance is None:
            args.consensus_tolerance = 0.05
        if not (math.isfinite(args.consensus_tolerance) and args.consensus_tolerance >= 0):
            ap.error("--consensus-tolerance takes seconds >= 0")
        if args.confidences:
            ap.error("--consensus and --confidences do not go together")
    if not args.velocities:
        for name in ("velocity_gamma", "velocity_anchor"):
            if getattr(args, name) is not None:
                ap.error("--%s needs --velocities" % name.replace("_", "-"))
    else:
        if args.model != "mt3":
            ap.error("--velocities is for --model mt3: ismir2021 decodes its velocities")
        for name in ("velocity_gamma", "velocity_anchor"):
            v = getattr(args, name)
            if v is not None and not (math.isfinite(v) and v > 0):
                ap.error("--%s takes a finite number > 0" % name.replace("_", "-"))
    if not args.harmony:
        if args.harmony_change_penalty is not None:
            ap.error("--harmony-change-penalty needs --harmony")
    else:
        args.beats = True
        if args.harmony_change_penalty is not None and not 0 <= args.harmony_change_penalty <= 1 << 20:
            ap.error("--harmony-change-penalty takes 0 .. 1048576")
    if not args.beats:
        for name in ("beats_prior_bpm", "quantize"):
            if getattr(args, name) is not None:
                ap.error("--%s needs --beats" % name.replace("_", "-"))
    else:
        if args.beats_prior_bpm is not None and not (math.isfinite(args.beats_prior_bpm) and args.beats_prior_bpm > 0):
            ap.error("--beats-prior-bpm takes a finite number > 0")
        if args.quantize is not None and not 1 <= args.quantize <= 48:
            ap.error("--quantize takes 1 .. 48 steps per beat")
    if (args.sustain or args.trim_overlaps) and args.score_against is None and args.score_midi is None and \
            args.align_midi is None and args.sync_midi is None:
        ap.error("--sustain and --trim-overlaps need --score-against, --score-midi, --align-midi or --sync-midi")
    for path in args.inputs:
        if not os.path.isfile(path):
            ap.error("no such file: %s" % path)
    if args.score_against is not None:
        for path in args.inputs:
            if not os.path.isfile(reference_path(args.score_against, path)):
                ap.error("--score-against: no such file: %s" % reference_path(args.score_against, path))
    if args.score_shifts is not None and args.score_midi is None:
        ap.error("--score-shifts needs --score-midi")
    if args.score_midi is not None:
        for path in args.inputs:
            if not os.path.isfile(reference_path(args.score_midi, path)):
                ap.error("--score-midi: no such file: %s" % reference_path(args.score_midi, path))
    if args.align_midi is None:
        for name in ("align_max_shift", "align_step", "align_smoothness"):
            if getattr(args, name) is not None:
                ap.error("--%s needs --align-midi" % name.replace("_", "-"))
    else:
        for path in args.inputs:
            if not os.path.isfile(reference_path(args.align_midi, path)):
                ap.error("--align-midi: no such file: %s" % reference_path(args.align_midi, path))
        max_shift = 0.2 if args.align_max_shift is None else args.align_max_shift
        step = 0.02 if args.align_step is None else args.align_step
        if not (math.isfinite(max_shift) and max_shift >= 0 and math.isfinite(step) and step > 0):
            ap.error("--align-max-shift takes seconds >= 0 and --align-step seconds > 0")
        if 2 * math.floor(max_shift / step + 1e-9) + 1 > 64:
            ap.error("--align-max-shift / --align-step: at most 64 shifts fit (a larger step, or a smaller maximum)")
        if args.align_smoothness is not None and not (math.isfinite(args.align_smoothness) and args.align_smoothness >= 0):
            ap.error("--align-smoothness takes a finite number >= 0")
        args.align_max_shift, args.align_step = max_shift, step
    if args.sync_midi is None:
        if args.sync_pool is not None:
            ap.error("--sync-pool needs --sync-midi")
    else:
        for path in args.inputs:
            if not os.path.isfile(reference_path(args.sync_midi, path)):
                ap.error("--sync-midi: no such file: %s" % reference_path(args.sync_midi, path))
        if args.sync_pool is not None and not 1 <= args.sync_pool <= 16:
            ap.error("--sync-pool takes 1 .. 16 log-mel frames")
    out = args.output
    if out is None:
        outputs = [os.path.splitext(p)[0] + ".mid" for p in args.inputs]
    elif len(args.inputs) == 1 and not os.path.isdir(out):
        outputs = [out]
    else:
        if os.path.exists(out) and not os.path.isdir(out):
            ap.error("-o %s is a file; %d inputs need a directory" % (out, len(args.inputs)))
        outputs = [os.path.join(out, os.path.splitext(os.path.basename(p))[0] + ".mid") for p in args.inputs]
    if len(set(os.path.abspath(p) for p in outputs)) != len(outputs):
        ap.error("two inputs would be written to the same output file")
    if args.score_against is not None and len(set(os.path.dirname(os.path.abspath(p)) for p in outputs)) != 1:
        ap.error("--score-against writes one scores.json into the output directory: inputs in several directories need -o DIR")
    if args.score_midi is not None and len(set(os.path.dirname(os.path.abspath(p)) for p in outputs)) != 1:
        ap.error("--score-midi writes one midi_scores.json into the output directory: inputs in several directories need -o DIR")
    if args.align_midi is not None and len(set(os.path.dirname(os.path.abspath(p)) for p in outputs)) != 1:
        ap.error("--align-midi writes one alignment.json into the output directory: inputs in several directories need -o DIR")
    if args.sync_midi is not None and len(set(os.path.dirname(os.path.abspath(p)) for p in outputs)) != 1:
        ap.error("--sync-midi writes one sync.json into the output directory: inputs in several directories need -o DIR")
    return args, outputs


def _shift_list(text: str):
    try:
        shifts = [float(v) for v in text.split(",") if v.strip() != ""]
    except ValueError:
        raise argparse.ArgumentTypeError("--score-shifts takes comma-separated seconds, got %r" % (text,)) from None
    if not shifts or any(not math.isfinite(v) for v in shifts):
        raise argparse.ArgumentTypeError("--score-shifts takes finite offsets in seconds, got %r" % (text,))
    return shifts


def _program_list(text: str):
    try:
        programs = [int(p) for p in text.split(",") if p.strip() != ""]
    except ValueError:
        raise argparse.ArgumentTypeError("--programs takes comma-separated integers, got %r" % (text,)) from None
    if not programs or any(not 0 <= p <= 127 for p in programs):
        raise argparse.ArgumentTypeError("--programs takes MIDI programs 0 .. 127, got %r" % (text,))
    return programs


def main(argv=None) -> int:
    args, outputs = plan(argv)
    from . import inference, midi_io
    try:
        model = inference.InferenceModel(args.checkpoint, args.model, dtype=args.dtype, decoding=args.decoding,
                                         num_beams=args.num_beams, temperature=args.temperature, top_k=args.top_k,
                                         top_p=args.top_p, seed=args.seed)
        votes = None
        velocities = velocity_keywords(args)
        if args.consensus is not None:
            from . import audio_io
            # every input file's N draws as ONE engine job (well_formed="tied" keeps its loop of N decodes)
            decoded = [audio_io.read_wav(path) for path in args.inputs]
            voted = model.consensus_many([s for s, _ in decoded], args.consensus, [r for _, r in decoded],
                                         tolerance=args.consensus_tolerance, min_votes=args.consensus_min_votes,
                                         return_votes=True, programs=args.programs, drums=args.drums,
                                         well_formed=args.well_formed)
            sequences, scores, votes = [ns for ns, _, _ in voted], None, [rec for _, rec, _ in voted]
            if velocities is not None:
                sequences = model.note_velocities_many(list(zip([s for s, _ in decoded], sequences)),
                                                       sample_rates=[r for _, r in decoded], **velocities)
        elif args.confidences:
            scored = [model.transcribe_wav_scored(path, programs=args.programs, drums=args.drums,
                                                  well_formed=args.well_formed)
                      for path in args.inputs]
            sequences, scores = [ns for ns, _ in scored], [sc for _, sc in scored]
            if velocities is not None:
                from . import audio_io
                decoded = [audio_io.read_wav(path) for path in args.inputs]
                sequences = model.note_velocities_many(list(zip([s for s, _ in decoded], sequences)),
                                                       sample_rates=[r for _, r in decoded], **velocities)
        else:
            sequences, scores = model.transcribe_wavs(args.inputs, programs=args.programs, drums=args.drums,
                                                      well_formed=args.well_formed, velocities=velocities), None
        found = None
        if args.beats:
            from . import beats
            # all inputs as one job, on the finished notes (whichever branch above made them)
            found = beats.track(sequences, **({} if args.beats_prior_bpm is None else {"prior_bpm": args.beats_prior_bpm}))
            if args.quantize is not None:
                sequences = beats.snap(sequences, found, args.quantize)
        analyzed = None
        if args.harmony:
            from . import harmony
            analyzed = harmony.analyze(sequences, found, **({} if args.harmony_change_penalty is None else
                                                            {"change_penalty": args.harmony_change_penalty}))
        rolls = None
        if args.pianoroll is not None:
            import numpy as np
            from . import pianoroll
            rolls = [r.clamp(0, 65535).to("cpu").numpy().astype(np.uint16)
                     for r in pianoroll.pianorolls(sequences, args.pianoroll)]
        audio = None
        if args.render is not None:
            from . import render
            written = [midi_io.midi_bytes_to_note_sequence(midi_io.note_sequence_to_midi_bytes(ns)) for ns in sequences]
            # (with --beats the file's ticks follow the tempo map; the render keeps the constant grid's rounding)
            audio = [a.cpu().numpy() for a in render.render(written, args.render)]
        scored = None
        if args.score_against is not None:
            from . import metrics
            references = known_notes(args.score_against, args)
            scored = metrics.transcription_metrics(list(zip(references, sequences)))
        midi_scores = None
        if args.score_midi is not None:
            from . import audio_io
            pairs, rates = [], []
            for path, ns in zip(args.inputs, known_notes(args.score_midi, args)):
                samples, rate = audio_io.read_wav(path)
                pairs.append((samples, ns))
                rates.append(rate)
            midi_scores = model.score_notes_many(pairs, sample_rates=rates, shifts=args.score_shifts)
        aligned = None
        if args.align_midi is not None:
            from . import audio_io
            pairs, rates = [], []
            for path, ns in zip(args.inputs, known_notes(args.align_midi, args)):
                samples, rate = audio_io.read_wav(path)
                pairs.append((samples, ns))
                rates.append(rate)
            aligned = model.align_notes_many(pairs, sample_rates=rates, max_shift=args.align_max_shift,
                                             step=args.align_step, smoothness=args.align_smoothness)
        synced = None
        if args.sync_midi is not None:
            from . import audio_io
            pairs, rates = [], []
            for path, ns in zip(args.inputs, known_notes(args.sync_midi, args)):
                samples, rate = audio_io.read_wav(path)
                pairs.append((samples, ns))
                rates.append(rate)
            synced = model.synchronize_many(pairs, sample_rates=rates,
                                            **({} if args.sync_pool is None else {"pool": args.sync_pool}))
    except Exception as e:                            # a file scipy cannot read, a checkpoint that does not load, ...
        print("mt3_amd.transcribe: %s: %s" % (type(e).__name__, e), file=sys.stderr)
        return 1
    for i, (ns, path) in enumerate(zip(sequences, outputs)):
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        mapped = found is not None and len(found[i].times) >= 2
        midi_io.note_sequence_to_midi_file(ns, path, beats=found[i].times if mapped else None,
                                           harmony=analyzed[i] if mapped and analyzed is not None else None)
        print("%s: %d notes" % (path, len(ns.notes)))
    for rec, path in zip(analyzed or [], outputs):
        with open(harmony_path(path), "w") as f:
            json.dump(harmony_record(rec), f, indent=1)
    for rec, path in zip(found or [], outputs):
        with open(beats_path(path), "w") as f:
            json.dump(beats_record(rec), f, indent=1)
    for ns, sc, path in zip(sequences, scores or [], outputs):
        with open(confidence_path(path), "w") as f:
            json.dump(confidence_records(ns, sc), f, indent=1)
    for rec, path in zip(votes or [], outputs):
        with open(votes_path(path), "w") as f:
            json.dump(votes_record(rec), f, indent=1)
    for roll, path in zip(rolls or [], outputs):
        import numpy as np
        np.save(pianoroll_path(path), roll)
    for samples, path in zip(audio or [], outputs):
        from . import audio_io
        with open(render_path(path), "wb") as f:
            f.write(audio_io.samples_to_wav_data(samples, args.render))
    if scored is not None:
        names = [os.path.splitext(os.path.basename(p))[0] for p in args.inputs]
        with open(scores_path(outputs), "w") as f:
            json.dump({"files": {name: {key: values[i] for key, values in scored["scores"].items()}
                                 for i, name in enumerate(names)}, "mean": scored["mean"]}, f, indent=1)
    if midi_scores is not None:
        with open(midi_scores_path(outputs), "w") as f:
            json.dump([midi_score_record(path, sc) for path, sc in zip(args.inputs, midi_scores)], f, indent=1)
    if aligned is not None:
        for rec, path in zip(aligned, outputs):
            midi_io.note_sequence_to_midi_file(rec["notes"], aligned_path(path))
        with open(alignment_path(outputs), "w") as f:
            json.dump([alignment_record(path, rec) for path, rec in zip(args.inputs, aligned)], f, indent=1)
    if synced is not None:
        for rec, path in zip(synced, outputs):
            midi_io.note_sequence_to_midi_file(rec["notes"], synced_path(path))
        with open(sync_json_path(outputs), "w") as f:
            json.dump([sync_record(path, rec) for path, rec in zip(args.inputs, synced)], f, indent=1)
    return 0


def synced_path(midi_path: str) -> str:
    return os.path.splitext(midi_path)[0] + ".synced.mid"


def sync_json_path(outputs) -> str:
    """sync.json of a job: beside scores.json"""
    return os.path.join(os.path.dirname(os.path.abspath(outputs[0])), "sync.json")


def sync_record(audio_path: str, rec) -> dict:
    """one JSON-ready record of `InferenceModel.synchronize`: the scores and the path thinned to one anchor per second of
    audio (the first cell at or after each whole second, and the last cell); the notes go to NAME.synced.mid"""
    audio, score = rec["path"]
    keep, second = [], -1
    for k, t in enumerate(audio):
        if int(t) > second:
            keep.append(k)
            second = int(t)
    if len(audio) and keep[-1] != len(audio) - 1:
        keep.append(len(audio) - 1)
    return {"audio": audio_path, "total": int(rec["total"]), "mean_cost": float(rec["mean_cost"]),
            "tempo_ratio": float(rec["tempo_ratio"]), "path": [[float(audio[k]), float(score[k])] for k in keep]}


def velocity_keywords(args):
    """--velocities [--velocity-gamma G --velocity-anchor V] -> the `velocities=` keyword of the model: None, or a dict"""
    if not args.velocities:
        return None
    named = {"gamma": args.velocity_gamma, "anchor_velocity": args.velocity_anchor}
    return {k: v for k, v in named.items() if v is not None}


def known_notes(directory: str, args) -> list:
    """DIR/NAME.mid of every input as a NoteSequence, prepared as --sustain / --trim-overlaps ask: one device job"""
    from . import midi_io
    sequences = []
    for path in args.inputs:
        with open(reference_path(directory, path), "rb") as f:
            sequences.append(midi_io.midi_bytes_to_note_sequence(f.read()))
    if args.sustain or args.trim_overlaps:
        from . import note_prep
        sequences = note_prep.prepare(sequences, sustain=args.sustain, trim=args.trim_overlaps)
    return sequences


def beats_path(midi_path: str) -> str:
    return os.path.splitext(midi_path)[0] + ".beats.json"


def beats_record(rec) -> dict:
    """the JSON-ready form of one `beats.Beats`"""
    return {"qpm": float(rec.qpm), "period_frames": int(rec.period), "beats": [float(t) for t in rec.times]}


def harmony_path(midi_path: str) -> str:
    return os.path.splitext(midi_path)[0] + ".harmony.json"


def harmony_record(rec) -> dict:
    """the JSON-ready form of one `harmony.Harmony`"""
    return {"key": int(rec.key), "key_name": rec.key_name, "sharps": int(rec.sharps), "beats_per_bar": int(rec.beats_per_bar),
            "downbeat": int(rec.downbeat), "downbeats": [float(t) for t in rec.downbeats],
            "chords": [[float(a), float(b), name] for a, b, name in rec.segments]}


def votes_path(midi_path: str) -> str:
    return os.path.splitext(midi_path)[0] + ".votes.json"


def votes_record(rec) -> dict:
    """the JSON-ready form of one `consensus.Consensus`: the notes in the NoteSequence's order with their votes"""
    return {"n_voters": rec.n_voters, "min_votes": rec.min_votes,
            "notes": [{"start_time": n.start_time, "end_time": n.end_time, "pitch": n.pitch, "program": n.program,
                       "is_drum": bool(n.is_drum), "votes": int(v), "members": int(m)}
                      for n, v, m in zip(rec.notes.notes, rec.votes, rec.members)]}


def aligned_path(midi_path: str) -> str:
    return os.path.splitext(midi_path)[0] + ".aligned.mid"


def alignment_path(outputs) -> str:
    """alignment.json of a job: beside scores.json"""
    return os.path.join(os.path.dirname(os.path.abspath(outputs[0])), "alignment.json")


def alignment_record(audio_path: str, rec) -> dict:
    """one JSON-ready record of `InferenceModel.align_notes`: the path and its scores (the notes go to NAME.aligned.mid)"""
    return {"audio": audio_path, "segment_shifts": [float(v) for v in rec["segment_shifts"]],
            "path_score": float(rec["path_score"]), "flat_shift": float(rec["flat_shift"]),
            "flat_score": float(rec["flat_score"])}


def midi_scores_path(outputs) -> str:
    """midi_scores.json of a job: beside scores.json"""
    return os.path.join(os.path.dirname(os.path.abspath(outputs[0])), "midi_scores.json")


def midi_score_record(audio_path: str, scores) -> dict:
    """one JSON-ready record of `InferenceModel.score_notes`: arrays as lists"""
    plain = (lambda v: v.tolist() if hasattr(v, "tolist") else v)
    return dict({"audio": audio_path}, **{k: plain(v) for k, v in scores.items()})


def reference_path(directory: str, wav_path: str) -> str:
    return os.path.join(directory, os.path.splitext(os.path.basename(wav_path))[0] + ".mid")


def scores_path(outputs) -> str:
    """scores.json of a job: in the directory its MIDI files are written to"""
    return os.path.join(os.path.dirname(os.path.abspath(outputs[0])), "scores.json")


def render_path(midi_path: str) -> str:
    return os.path.splitext(midi_path)[0] + ".render.wav"


def pianoroll_path(midi_path: str) -> str:
    return os.path.splitext(midi_path)[0] + ".npy"


def confidence_path(midi_path: str) -> str:
    return os.path.splitext(midi_path)[0] + ".confidence.json"


def confidence_records(ns, scores):
    """one JSON-ready record per note of `ns`, in its order: the note's fields and its three confidences (NaN -> None)"""
    num = (lambda v: None if math.isnan(v) else float(v))
    return [{"start_time": n.start_time, "end_time": n.end_time, "pitch": n.pitch, "velocity": n.velocity,
             "program": n.program, "is_drum": bool(n.is_drum), "instrument": n.instrument,
             "onset_logprob": num(scores["onset_logprob"][i]), "end_logprob": num(scores["end_logprob"][i]),
             "onset_margin": num(scores["onset_margin"][i])}
            for i, n in enumerate(ns.notes)]


if __name__ == "__main__":
    sys.exit(main())
