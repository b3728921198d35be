"""Entry points: CLI parsing / schedules / logger on CPU, and a short run of each CLI on the GPU."""
import json
import os

import numpy as np
import pytest


def test_dllogger_format(tmp_path):
    from deeplearningexamples_amd.utils import dllogger
    f = tmp_path / "log.json"
    dllogger.init([dllogger.JSONStreamBackend(dllogger.Verbosity.VERBOSE, str(f))])
    dllogger.metadata("train.loss", {"unit": None})
    dllogger.log(step=(0, 3), data={"train.loss": 1.5, "train.total_ips": 100.0})
    dllogger.flush()
    lines = open(f).read().strip().splitlines()
    assert all(l.startswith("DLLL ") for l in lines)
    rec = json.loads(lines[-1][5:])
    assert rec["type"] == "LOG" and rec["step"] == [0, 3] and rec["data"]["train.loss"] == 1.5


def test_rn50_lr_policies_match_reference_formulas():
    # optimizers.py:82-130 evaluated by hand
    from deeplearningexamples_amd.convnets.engine import lr_cosine_policy, lr_linear_policy, lr_step_policy
    cos = lr_cosine_policy(2.048, 8, 250)
    assert cos(0, 0) == pytest.approx(2.048 / 8) and cos(0, 7) == pytest.approx(2.048)
    assert cos(0, 129) == pytest.approx(0.5 * (1 + np.cos(np.pi * 121 / 242)) * 2.048)
    step = lr_step_policy(0.1, [30, 60, 80], 0.1, 5)
    assert step(0, 2) == pytest.approx(0.06) and step(0, 65) == pytest.approx(0.001)
    lin = lr_linear_policy(1.0, 2, 12)
    assert lin(0, 7) == pytest.approx(0.5)


def test_cli_parsers():
    from deeplearningexamples_amd.convnets.main import add_parser_arguments
    import argparse
    a = add_parser_arguments(argparse.ArgumentParser()).parse_args(
        ["--arch", "resnet50", "-b", "64", "--amp", "--label-smoothing", "0.1", "--lr-schedule", "cosine", "--warmup", "8"])
    assert a.batch_size == 64 and a.amp and a.lr_schedule == "cosine"
    from deeplearningexamples_amd.bert.run_pretraining import parse_arguments
    b = parse_arguments(["--train_batch_size", "64", "--gradient_accumulation_steps", "4", "--max_steps", "10", "--bf16"])
    assert b.steps_this_run == 10 and b.train_batch_size // b.gradient_accumulation_steps == 16
    with pytest.raises(ValueError):
        parse_arguments(["--train_batch_size", "10", "--gradient_accumulation_steps", "4"])
    from deeplearningexamples_amd.dlrm.main import parse_flags
    f = parse_flags(["--top_mlp_sizes", "64,32,1", "--synthetic_dataset_table_sizes", "100,200", "--amp", "--dataset_type",
                     "synthetic_gpu"])
    assert f.top_mlp_sizes == [64, 32, 1] and f.synthetic_dataset_table_sizes == [100, 200] and f.amp


def test_dlrm_flags_follow_absl_boolean_syntax_and_the_reference_defaults():
    """dlrm/scripts/main.py:43-143 defines its flags with absl: booleans are written --amp, --noamp or --amp=True|False (the
    reference's own test scripts use the last form, tests/test_all_configs.sh:17-27); --dataset_type defaults to parametric,
    --embedding_type to custom_cuda, the synthetic table sizes to 26 x 100000, --optimized_mlp to True."""
    from deeplearningexamples_amd.dlrm.main import parse_flags
    f = parse_flags(["--mode", "train", "--dataset", "/d", "--optimized_mlp=False", "--cuda_graphs=True", "--interaction_op=dot",
                     "--embedding_type=joint_sparse", "--amp=False", "--hash_indices", "--noshuffle"])
    assert (f.optimized_mlp, f.cuda_graphs, f.amp, f.hash_indices, f.shuffle_batch_order) == (False, True, False, True, False)
    assert f.dataset_type == "parametric" and f.embedding_type == "joint_sparse" and f.interaction_op == "dot"
    d = parse_flags(["--dataset", "/d"])
    assert d.embedding_type == "custom_cuda" and d.synthetic_dataset_table_sizes == 26 * [100000] and d.optimized_mlp is True
    assert d.amp is False and d.cuda_graphs is False and d.lr == 24 and d.batch_size == 65536
    s = parse_flags(["--dataset_type=synthetic_gpu", "--amp=1", "--shuffle", "--nooptimized_mlp", "--freeze_mlps=t"])
    assert s.amp is True and s.shuffle_batch_order is True and s.optimized_mlp is False and s.freeze_mlps is True
    for bad in (["--dataset", "/d", "--amp=maybe"], [], ["--dataset", "/d", "--interaction_op=cat"],
                ["--dataset_type=synthetic_gpu", "--synthetic_dataset_use_feature_spec"]):
        with pytest.raises(SystemExit):
            parse_flags(bad)


def test_reference_command_lines_parse():
    """The reference's own command lines (README / scripts) must not end in an argparse error: every flag of
    ConvNets/main.py:89-356, run_pretraining.py:140-321 and dlrm/scripts/main.py:43-143 is known to the drop-in parsers."""
    import argparse
    from deeplearningexamples_amd.convnets.main import add_parser_arguments
    from deeplearningexamples_amd.bert.run_pretraining import parse_arguments
    from deeplearningexamples_amd.dlrm.main import parse_flags
    a = add_parser_arguments(argparse.ArgumentParser()).parse_args(
        ["--arch", "resnet50", "-b", "256", "--amp", "--static-loss-scale", "128", "--label-smoothing", "0.1", "--mixup", "0.2",
         "--lr", "2.048", "--lr-schedule", "cosine", "--warmup", "8", "--epochs", "250", "--momentum", "0.875", "--wd", "3.05e-5",
         "--resume", "ck/checkpoint.pth.tar", "--checkpoint-filename", "c.pth.tar", "--gather-checkpoints", "3", "--evaluate",
         "--data-backend", "pytorch", "--memory-format", "nhwc", "--workspace", "/tmp/w", "--raport-file", "r.json", "-j", "8",
         "--run-epochs", "2", "--training-only", "--no-checkpoints", "--topk", "5", "--seed", "1", "/data/imagenet"])
    assert a.data == "/data/imagenet" and a.resume and a.gather_checkpoints == 3 and not a.save_checkpoints
    b = parse_arguments(["--input_dir", "/d", "--output_dir", "/o", "--config_file", "bert_config.json", "--bert_model",
                         "bert-large-uncased", "--train_batch_size", "8192", "--max_seq_length", "512",
                         "--max_predictions_per_seq", "80", "--max_steps", "1563", "--warmup_proportion", "0.128",
                         "--num_steps_per_checkpoint", "200", "--learning_rate", "4e-3", "--seed", "42", "--fp16",
                         "--gradient_accumulation_steps", "256", "--allreduce_post_accumulation",
                         "--allreduce_post_accumulation_fp16", "--do_train", "--phase2", "--resume_from_checkpoint",
                         "--phase1_end_step", "7038", "--json-summary", "j.json", "--disable_progress_bar", "--num_workers", "4",
                         "--init_checkpoint", "x.pt", "--resume_step", "7038", "--cuda_graphs", "--use_env"])
    assert b.phase2 and b.resume_from_checkpoint and b.num_steps_per_checkpoint == 200 and b.output_dir == "/o"
    f = parse_flags(["--dataset", "/data", "--seed", "1", "--epochs", "1", "--amp", "--cuda_graphs", "--save_checkpoint_path",
                     "/ck", "--load_checkpoint_path", "/ck", "--test_freq", "100", "--test_after", "0.5", "--auc_threshold",
                     "0.8025", "--test_batch_size", "131072", "--mode", "test", "--dataset_type", "parametric"])
    assert f.auc_threshold == 0.8025 and f.test_freq == 100 and f.save_checkpoint_path == "/ck" and f.mode == "test"
    # every flag the reference defines is accepted here (flag NAMES; semantics: the GPU test below).  The reference's flag names are
    # stored in tests/golden/reference_interfaces.json (oracle/make_golden.py reference_interfaces reads them out of its sources)
    names = _reference_interfaces()["flag_names"]
    ours = {"rn50": add_parser_arguments(argparse.ArgumentParser())}
    known = {o for act in ours["rn50"]._actions for o in act.option_strings}
    missing = [x for x in names["convnets"] if x not in known]
    assert not missing, missing
    import deeplearningexamples_amd.bert.run_pretraining as bp
    psrc = open(bp.__file__).read()
    missing = [x for x in names["bert"] if '"%s"' % x not in psrc]
    assert not missing, missing
    flags = names["dlrm"]
    import deeplearningexamples_amd.dlrm.main as dm
    known = {o for act in dm.build_parser()._actions for o in act.option_strings}
    missing = [x for x in flags if "--" + x not in known]
    assert not missing and len(flags) >= 45, (missing, len(flags))
    # absl gives every boolean flag a --no<name> twin (and shuffle_batch_order the short name --shuffle)
    booleans = names["dlrm_booleans"]
    assert len(booleans) >= 10 and not [x for x in booleans if "--no" + x not in known] and "--shuffle" in known
    # SpeechSynthesis/Tacotron2: train.py:45-160 + tacotron2/arg_parser.py:40-107 + waveglow/arg_parser.py:30-64
    from deeplearningexamples_amd.tacotron2 import train as t2
    from deeplearningexamples_amd.waveglow import train as wg
    for mod, key in ((t2, "tacotron2"), (wg, "waveglow")):
        flags = names[key]
        known = _known_flags(mod)
        missing = sorted(x for x in flags if x not in known)
        assert not missing and len(flags) > 50 - 10 * (mod is wg), (mod.__name__, missing, len(flags))


def _reference_interfaces():
    """tests/golden/reference_interfaces.json; a keyword whose value is an expression in the reference's sources reads as Ellipsis."""
    here = os.path.dirname(os.path.abspath(__file__))
    return json.load(open(os.path.join(here, "golden", "reference_interfaces.json")),
                     object_hook=lambda d: {k: Ellipsis if v == "<expression>" else v for k, v in d.items()})


def _known_flags(mod):
    """Option strings of the parser `mod.parse_args` builds (captured without parsing a command line)."""
    import argparse
    seen = {}
    real = argparse.ArgumentParser.parse_known_args

    def grab(self, args=None, namespace=None):
        seen["p"] = self
        return real(self, args, namespace)

    argparse.ArgumentParser.parse_known_args = grab
    try:
        mod.parse_args(["-o", "x", "-lr", "1", "--epochs", "1", "-bs", "1"])
    finally:
        argparse.ArgumentParser.parse_known_args = real
    return {o for act in seen["p"]._actions for o in act.option_strings}


def _captured_parser(fn, argv):
    """The argparse parser `fn(argv)` builds, captured at its parse call."""
    import argparse
    seen = {}
    real, real_known = argparse.ArgumentParser.parse_args, argparse.ArgumentParser.parse_known_args

    def grab_known(self, args=None, namespace=None):
        seen.setdefault("p", self)
        return real_known(self, args, namespace)

    def grab(self, args=None, namespace=None):
        seen.setdefault("p", self)
        return real(self, args, namespace)

    argparse.ArgumentParser.parse_args, argparse.ArgumentParser.parse_known_args = grab, grab_known
    try:
        fn(argv)
    finally:
        argparse.ArgumentParser.parse_args, argparse.ArgumentParser.parse_known_args = real, real_known
    return seen["p"]


def test_flag_defaults_choices_and_kinds_match_the_reference_sources():
    """Same names is not yet a drop-in: every flag's DEFAULT, its choices and whether it is a switch, as the reference's sources
    define them (ast over the add_argument / absl DEFINE_* calls of ConvNets/main.py, BERT/run_pretraining.py, Tacotron2/train.py +
    arg_parser.py files, DLRM/dlrm/scripts/main.py; stored in tests/golden/reference_interfaces.json by oracle/make_golden.py), are
    compared with the parsers here.  The deviations are the ones listed."""
    import argparse
    ref = _reference_interfaces()["flags"]

    def check(title, flags, parser, allowed):
        mine = {o: a for a in parser._actions for o in a.option_strings}
        bad = []
        for name, kw in sorted(flags.items()):
            a = mine.get(name)
            if a is None:
                bad.append((name, "missing"))
                continue
            switch = kw.get("action") in ("store_true", "store_false")
            if switch != (a.nargs == 0):
                bad.append((name, "switch" if switch else "takes a value"))
            want = kw.get("default", False if kw.get("action") == "store_true" else (True if kw.get("action") == "store_false" else None))
            if want is not Ellipsis and name not in allowed and want != a.default and not (want is None and a.default is False):
                bad.append((name, "default", want, a.default))
            ch = kw.get("choices")
            if ch not in (None, Ellipsis) and (a.choices is None or list(ch) != list(a.choices)):
                bad.append((name, "choices", ch, a.choices))
        assert not bad, (title, bad)
        return len(flags)

    from deeplearningexamples_amd.convnets.main import add_parser_arguments
    n = check("convnets", ref["convnets"], add_parser_arguments(argparse.ArgumentParser()),
              # no DALI on ROCm: the synthetic loader is the default backend; 224 is what the reference fills in for resnet50 when
              # --image-size is None; "0" / 0
              {"--data-backend", "--image-size", "--gather-checkpoints"})
    assert n >= 40
    import deeplearningexamples_amd.bert.run_pretraining as bp
    n = check("bert", ref["bert"], _captured_parser(bp.parse_arguments, ["--bf16"]), set())
    assert n >= 40
    from deeplearningexamples_amd.tacotron2 import train as t2
    from deeplearningexamples_amd.waveglow import train as wg
    argv = ["-o", "x", "-lr", "1", "--epochs", "1", "-bs", "1"]
    for mod, key in ((t2, "tacotron2"), (wg, "waveglow")):
        # one entry point per model here: --model-name defaults to it (required, no default, in the reference's shared train.py)
        n = check(mod.__name__, ref[key], _captured_parser(mod.parse_args, argv), {"--model-name"})
        assert n >= 40
    # DLRM: absl DEFINE_<kind>(name, default, ...)
    from deeplearningexamples_amd.dlrm.main import build_parser
    mine = {o: a for a in build_parser()._actions for o in a.option_strings}
    bad, seen = [], 0
    for d in ref["dlrm"]:
        kind, name, default = d["kind"], d["name"], d["default"]
        a = mine.get("--" + name)
        seen += 1
        if a is None:
            bad.append((name, "missing"))
            continue
        if kind == "list" and isinstance(default, str):
            default = default.split(",")
        if kind == "list" and default is not Ellipsis:
            default = [int(x) for x in default]
        if kind == "integer" and isinstance(default, str):
            default = int(default)
        if default is not Ellipsis and default != a.default:
            bad.append((name, "default", default, a.default))
        if kind == "enum":
            ch = d["choices"]
            if ch is not Ellipsis and list(ch) != list(a.choices):
                bad.append((name, "choices", ch, a.choices))
        if kind == "boolean" and ("--no" + name not in mine or a.nargs != "?"):
            bad.append((name, "not an absl boolean"))
    assert not bad and seen >= 45, (bad, seen)


def test_speech_command_lines_parse_and_config_file(tmp_path):
    """scripts/train_tacotron2.sh / train_waveglow.sh of the reference + --config-file (tacotron2_common/utils.py:36-49)."""
    from deeplearningexamples_amd.tacotron2 import train as t2
    from deeplearningexamples_amd.waveglow import train as wg
    a = t2.parse_args("-m Tacotron2 -o ./output/ -lr 1e-3 --epochs 1501 -bs 48 --weight-decay 1e-6 --grad-clip-thresh 1.0 "
                      "--cudnn-enabled --log-file nvlog.json --anneal-steps 500 1000 1500 --anneal-factor 0.1 --load-mel-from-disk "
                      "--training-files filelists/ljs_mel_text_train_filelist.txt --validation-files filelists/ljs_mel_text_val_filelist.txt "
                      "-d /data/LJSpeech-1.1 --mask-padding True --text-cleaners english_cleaners --resume-from-last".split())
    assert a.load_mel_from_disk and a.mask_padding and a.dataset_path == "/data/LJSpeech-1.1" and not a.synthetic_data
    assert t2.get_model_config(a)["mask_padding"] is True and set(t2.get_model_config(a)) >= {"max_decoder_steps", "gate_threshold"}
    b = wg.parse_args("-m WaveGlow -o ./output/ -lr 1e-4 --epochs 1501 -bs 4 --segment-length 8000 --weight-decay 0 "
                      "--grad-clip-thresh 3.4028234663852886e+38 --cudnn-enabled --cudnn-benchmark --log-file nvlog.json".split())
    assert b.segment_length == 8000 and b.grad_clip_thresh > 3e38 and b.training_files.endswith("ljs_audio_text_train_filelist.txt")
    cfg = tmp_path / "config.json"
    cfg.write_text(json.dumps({"audio": {"sampling-rate": 16000, "hop-length": 200}, "model": {"prenet-dim": 128}}))
    c = t2.parse_args(["-o", "x", "-lr", "1", "--epochs", "1", "-bs", "1", "--config-file", str(cfg)])
    assert (c.sampling_rate, c.hop_length, c.prenet_dim) == (16000, 200, 128)


def _speech_dataset(root, n_train=6, n_val=3, mels=True):
    """A tiny LJSpeech-shaped dataset: 22.05 kHz int16 wavs, saved mels, `path|text` filelists."""
    import torch
    from scipy.io.wavfile import write
    rng = np.random.default_rng(0)
    os.makedirs(root / "wavs"), os.makedirs(root / "mels"), os.makedirs(root / "filelists")
    words = "the quick brown fox jumps over a lazy dog while printing differs from most arts".split()
    for split, n in (("train", n_train), ("val", n_val)):
        la, lm = [], []
        for i in range(n):
            name = "%s%d" % (split, i)
            samples = int(rng.integers(5000, 9000))
            write(str(root / "wavs" / (name + ".wav")), 22050, (rng.standard_normal(samples) * 6000).astype(np.int16))
            torch.save(torch.randn(80, int(rng.integers(18, 40))) * 1.5 - 4.0, str(root / "mels" / (name + ".pt")))
            text = " ".join(rng.choice(words, int(rng.integers(3, 8)))).capitalize() + "."
            la.append("wavs/%s.wav|%s" % (name, text))
            lm.append("mels/%s.pt|%s" % (name, text))
        (root / "filelists" / ("audio_%s.txt" % split)).write_text("\n".join(la) + "\n")
        (root / "filelists" / ("mel_%s.txt" % split)).write_text("\n".join(lm) + "\n")


@pytest.mark.gpu
def test_speech_entry_points_train_validate_and_resume_from_filelists(cuda, tmp_path):
    """the Tacotron2 and WaveGlow CLIs on a tiny on-disk dataset -- TextMelLoader (saved mels and wavs
    through the STFT front end) + TextMelCollate, MelAudioLoader, --mask-padding, the per-epoch validation pass, checkpoint + resume."""
    from deeplearningexamples_amd.tacotron2 import train as t2
    from deeplearningexamples_amd.waveglow import train as wg
    data = tmp_path / "data"
    _speech_dataset(data)
    small = ("--symbols-embedding-dim 64 --encoder-embedding-dim 64 --attention-rnn-dim 96 --attention-dim 32 "
             "--attention-location-n-filters 8 --decoder-rnn-dim 96 --prenet-dim 48 --postnet-embedding-dim 64").split()
    out = tmp_path / "t2"
    common = ["-m", "Tacotron2", "-o", str(out), "-d", str(data), "--amp", "-lr", "1e-3", "-bs", "2", "--seed", "3",
              "--epochs-per-checkpoint", "1", "--mask-padding", "True", "--text-cleaners", "english_cleaners"] + small
    mel_lists = ["--load-mel-from-disk", "--training-files", "filelists/mel_train.txt", "--validation-files", "filelists/mel_val.txt"]
    t2.main(common + mel_lists + ["--epochs", "2"])
    recs = [json.loads(l[5:]) for l in open(out / "nvlog.json")]
    val = [r["data"]["val_loss"] for r in recs if r["type"] == "LOG" and "val_loss" in r.get("data", {}) and r["step"] not in ([],)]
    tl = [r["data"]["train_loss"] for r in recs if r["type"] == "LOG" and "train_loss" in r.get("data", {}) and len(r["step"]) == 2]
    assert len(tl) == 2 * 3 and len(val) >= 2 and all(np.isfinite(v) for v in val + tl)          # 6 files / bs 2 x 2 epochs
    assert os.path.islink(out / "checkpoint_Tacotron2_last.pt") and os.path.exists(out / "checkpoint_Tacotron2_1.pt")
    import torch
    ck = torch.load(out / "checkpoint_Tacotron2_1.pt", map_location="cpu", weights_only=False)
    assert ck["config"]["mask_padding"] is True and ck["epoch"] == 1
    t2.main(common + mel_lists + ["--epochs", "3", "--resume-from-last"])                         # one more epoch from the link
    recs2 = [json.loads(l[5:]) for l in open(out / "nvlog.json")]
    assert any(r.get("step") == [2, 0] for r in recs2) and os.path.exists(out / "checkpoint_Tacotron2_2.pt")
    # wavs through the STFT front end
    out_w = tmp_path / "t2w"
    t2.main(["-m", "Tacotron2", "-o", str(out_w), "-d", str(data), "--amp", "-lr", "1e-3", "-bs", "3", "--epochs", "1",
             "--training-files", "filelists/audio_train.txt", "--validation-files", "filelists/audio_val.txt"] + small)
    recs = [json.loads(l[5:]) for l in open(out_w / "nvlog.json")]
    assert sum("train_loss" in r.get("data", {}) and len(r.get("step", [])) == 2 for r in recs) == 2
    # WaveGlow
    out_g = tmp_path / "wg"
    wg_small = "--flows 4 --wn-layers 2 --wn-channels 64 --early-every 2 --segment-length 2048".split()
    wg.main(["-m", "WaveGlow", "-o", str(out_g), "-d", str(data), "--amp", "-lr", "1e-4", "-bs", "2", "--epochs", "1", "--weight-decay", "0",
             "--grad-clip-thresh", "65504.0", "--training-files", "filelists/audio_train.txt", "--validation-files",
             "filelists/audio_val.txt"] + wg_small)
    recs = [json.loads(l[5:]) for l in open(out_g / "nvlog.json")]
    assert sum("train_loss" in r.get("data", {}) and len(r.get("step", [])) == 2 for r in recs) == 3
    assert any("val_loss" in r.get("data", {}) for r in recs) and os.path.exists(out_g / "checkpoint_WaveGlow_0.pt")
    # synthetic mode + missing filelist
    wg.main(["-o", str(tmp_path / "wgs"), "-lr", "1e-4", "-bs", "2", "--epochs", "1", "--amp", "--synthetic-data", "--iters-per-epoch", "2"] + wg_small)
    with pytest.raises(SystemExit, match="no such filelist"):
        t2.main(["-o", str(tmp_path / "none"), "-lr", "1e-3", "-bs", "2", "--epochs", "1"] + small)


@pytest.mark.gpu
def test_entry_points_save_and_resume_on_gpu(cuda, tmp_path):
    """f2 / f4 through the drop-in command lines: each CLI trains, writes the reference's checkpoint file(s), a SECOND process-
    equivalent call resumes from them and continues; the ResNet CLI evaluates (--evaluate), the DLRM CLI logs an AUC."""
    import torch
    from deeplearningexamples_amd.convnets import main as rn
    from deeplearningexamples_amd.bert import run_pretraining as bp
    from deeplearningexamples_amd.dlrm import main as dl
    # ---- ResNet-50: 2 epochs of 3 iterations with validation and checkpoints, then resume for a third epoch, then --evaluate
    ws = tmp_path / "rn"
    common = ["--batch-size", "8", "--image-size", "64", "--prof", "3", "--amp", "--label-smoothing", "0.1", "--lr", "0.01",
              "--lr-schedule", "cosine", "--warmup", "1", "--workspace", str(ws), "--print-freq", "1", "--steps-per-epoch", "3",
              "--num-classes", "16", "--seed", "3"]
    rn.main(common + ["--epochs", "3", "--run-epochs", "2"])
    assert {"checkpoint.pth.tar", "checkpoint_0000.pth.tar", "checkpoint_0001.pth.tar"} <= set(os.listdir(ws))
    ck = torch.load(ws / "checkpoint.pth.tar", map_location="cpu", weights_only=False)
    assert ck["epoch"] == 2 and set(ck) >= {"state_dict", "optimizer", "best_prec1"}
    t = rn.main(common + ["--epochs", "3", "--resume", str(ws / "checkpoint.pth.tar")])
    assert (ws / "checkpoint_0002.pth.tar").exists() and t.steps_done == 9          # 6 restored + 3 new iterations
    recs = [json.loads(l[5:]) for l in open(ws / "experiment_raport.json")]
    assert any("val.top1" in r.get("data", {}) for r in recs)
    rn.main(common + ["--epochs", "3", "--resume", str(ws / "checkpoint_0001.pth.tar"), "--evaluate"])
    # mixup + nhwc loader batches run through the same CLI
    rn.main(common + ["--epochs", "1", "--mixup", "0.2", "--memory-format", "nhwc", "--no-checkpoints", "--training-only",
                      "--workspace", str(tmp_path / "rn2")])
    # ---- ResNet-50, --data-backend pytorch over a folder of pre-decoded images (uint8 -> normalised NHWC in the first kernel)
    rng = np.random.default_rng(0)
    for split in ("train", "val"):
        for c in range(2):
            d = tmp_path / "imgs" / split / ("class%d" % c)
            os.makedirs(d)
            for i in range(8):
                np.save(d / ("%d.npy" % i), rng.integers(0, 256, (80, 96, 3), dtype=np.uint8))
    rn.main(["--batch-size", "4", "--image-size", "64", "--epochs", "1", "--amp", "--lr", "0.01", "--workspace",
             str(tmp_path / "rn3"), "--data-backend", "pytorch", "--num-classes", "2", "--topk", "2", "-j", "0", "--print-freq", "1",
             str(tmp_path / "imgs")])
    recs = [json.loads(l[5:]) for l in open(tmp_path / "rn3" / "experiment_raport.json")]
    assert any("val.top1" in r.get("data", {}) for r in recs) and any("train.loss" in r.get("data", {}) for r in recs)
    # ---- BERT: 4 steps with a checkpoint every 2, "killed" after 4; resume to 6; phase-2 restart from the phase-1 file
    cfg = tmp_path / "tiny.json"
    cfg.write_text(json.dumps(dict(vocab_size=1000, hidden_size=256, num_attention_heads=4, num_hidden_layers=2,
                                   intermediate_size=1024, max_position_embeddings=512, type_vocab_size=2)))
    out = tmp_path / "bert_out"
    base = ["--config_file", str(cfg), "--train_batch_size", "8", "--gradient_accumulation_steps", "2", "--max_steps", "6",
            "--max_seq_length", "128", "--max_predictions_per_seq", "20", "--learning_rate", "6e-3", "--warmup_proportion", "0.2843",
            "--json-summary", str(tmp_path / "bert.json"), "--bf16", "--output_dir", str(out), "--num_steps_per_checkpoint", "2",
            "--do_train"]
    t = bp.main(base + ["--steps_this_run", "4"])
    assert sorted(os.listdir(out)) == ["ckpt_2.pt", "ckpt_4.pt"] and t.opt_steps == 4
    w4 = t.model.state_dict()["bert.pooler.dense_act.weight"].clone()
    t2 = bp.main(base + ["--resume_from_checkpoint"])
    assert t2.opt_steps == 6 and sorted(os.listdir(out)) == ["ckpt_2.pt", "ckpt_4.pt", "ckpt_6.pt"]
    ck = torch.load(out / "ckpt_4.pt", map_location="cpu", weights_only=False)
    assert torch.equal(ck["model"]["bert.pooler.dense_act.weight"].cpu(), w4.cpu()) and int(ck["optimizer"]["param_groups"][0]["step"]) == 4
    t3 = bp.main(base[:-5] + ["--output_dir", str(tmp_path / "bert_p2"), "--init_checkpoint", str(out / "ckpt_6.pt"), "--phase2",
                              "--max_seq_length", "256", "--max_predictions_per_seq", "40", "--steps_this_run", "2"])
    assert t3.opt_steps == 2                       # step and LR restart (run_pretraining.py:437-445)
    # ---- DLRM: train with validation passes + save; test mode from the saved directory; resume training from it
    ckd = tmp_path / "dlrm_ck"
    dbase = ["--dataset_type", "synthetic_gpu", "--batch_size", "2048", "--synthetic_dataset_table_sizes", "1000,50,7,20000", "--amp",
             "--print_freq", "2",
             "--synthetic_dataset_num_entries", "16384", "--test_batch_size", "4096"]
    dl.main(dbase + ["--max_steps", "6", "--log_path", str(tmp_path / "dlrm.json"), "--test_freq", "3",
                     "--save_checkpoint_path", str(ckd)])
    recs = [json.loads(l[5:]) for l in open(tmp_path / "dlrm.json")]
    aucs = [r["data"]["auc"] for r in recs if "auc" in r.get("data", {})]
    assert aucs and all(0.0 <= a <= 1.0 for a in aucs) and "best_auc" in recs[-1]["data"]
    assert os.path.exists(ckd / "metadata.pt") and os.path.exists(ckd / "bottom_model.embeddings.0.bin")
    dl.main(dbase + ["--mode", "test", "--load_checkpoint_path", str(ckd), "--log_path", str(tmp_path / "dlrm_test.json")])
    rt = [json.loads(l[5:]) for l in open(tmp_path / "dlrm_test.json")]
    assert rt[-1]["data"]["best_auc"] == pytest.approx(aucs[-1], abs=0.05)     # same weights up to the steps after the last test
    t = dl.main(dbase + ["--max_steps", "3", "--load_checkpoint_path", str(ckd), "--log_path", str(tmp_path / "dlrm2.json")])
    assert t is not None


@pytest.mark.gpu
def test_entry_points_run_on_gpu(cuda, tmp_path):
    from deeplearningexamples_amd.convnets import main as rn
    from deeplearningexamples_amd.bert import run_pretraining as bp
    from deeplearningexamples_amd.dlrm import main as dl
    rn.main(["--batch-size", "8", "--image-size", "64", "--epochs", "1", "--prof", "3", "--amp", "--label-smoothing", "0.1",
             "--lr", "0.01", "--lr-schedule", "cosine", "--warmup", "1", "--workspace", str(tmp_path), "--print-freq", "1"])
    recs = [json.loads(l[5:]) for l in open(tmp_path / "experiment_raport.json")]
    assert any("train.loss" in r.get("data", {}) for r in recs) and "train.total_ips" in recs[-1]["data"]
    cfg = tmp_path / "tiny.json"
    cfg.write_text(json.dumps(dict(vocab_size=1000, hidden_size=256, num_attention_heads=4, num_hidden_layers=2,
                                   intermediate_size=1024, max_position_embeddings=512, type_vocab_size=2)))
    t = bp.main(["--config_file", str(cfg), "--train_batch_size", "8", "--gradient_accumulation_steps", "2", "--max_steps", "3",
                 "--max_seq_length", "128", "--max_predictions_per_seq", "20", "--json-summary", str(tmp_path / "bert.json"), "--bf16"])
    recs = [json.loads(l[5:]) for l in open(tmp_path / "bert.json")]
    assert "training_sequences_per_second" in recs[-1]["data"] and t.opt_steps == 3
    dl.main(["--dataset_type", "synthetic_gpu", "--batch_size", "2048", "--synthetic_dataset_table_sizes", "1000,50,7,20000",
             "--max_steps", "5", "--amp",
             "--log_path", str(tmp_path / "dlrm.json"), "--print_freq", "2", "--synthetic_dataset_num_entries", "16384"])
    recs = [json.loads(l[5:]) for l in open(tmp_path / "dlrm.json")]
    assert "average_train_throughput" in recs[-1]["data"]


def test_bert_lr_schedule_matches_reference_scheduler():
    """bert.engine.poly_warmup_lr == the oracle's restatement == the stored learning rates of the reference's
    own PolyWarmUpScheduler stepped on a dummy optimizer (LanguageModeling/BERT/schedulers.py:109-136)."""
    from deeplearningexamples_amd.bert.engine import poly_warmup_lr
    from oracle import bert_oracle as BO
    base, warm, total = 6e-3, 0.2843, 40
    ours = [poly_warmup_lr(s, base, warm, total) for s in range(1, total)]
    orc = [BO.poly_warmup_lr(s, base, warm, total) for s in range(1, total)]
    assert max(abs(a - b) for a, b in zip(ours, orc)) < 1e-12
    assert poly_warmup_lr(total + 5, base, warm, total) == 0.0
    # the reference's PolyWarmUpScheduler stepped for k = 0..10 completed steps (run_pretraining.py:529 steps the scheduler BEFORE the
    # optimizer; FusedLAMBAMP keeps the completed-step count in param_group["step"]), stored by oracle/make_golden.py
    ref = _reference_interfaces()["bert_poly_warmup_lr"]
    assert (ref["base_lr"], ref["warmup"], ref["total_steps"]) == (base, warm, total)
    assert max(abs(a - b) for a, b in zip(ref["lr"], ours[:11])) < 1e-9 and len(ref["lr"]) == 11


def test_flags_without_effect_are_reported_and_unknown_speech_flags_are_warned_about():
    """A flag that parses must not silently do nothing (run_pretraining.py:557-570 --input_dir feeds the lddl loader in the reference;
    here the batches are synthetic and the run says so).  The contract for UNKNOWN flags differs by entry point, as in the
    reference: BERT's argparse rejects them (parse_args, run_pretraining.py:120-291); the two speech CLIs parse like the reference
    (Tacotron2/train.py:349,382 parse_known_args: a command line shared by both models or a launcher's --local_rank must not
    abort the run) -- unknown flags there are NOT errors, they are named in a warning on stderr."""
    from deeplearningexamples_amd.bert import run_pretraining as bp
    from deeplearningexamples_amd.tacotron2 import train as t2
    from deeplearningexamples_amd.waveglow import train as wg
    a = bp.parse_arguments(["--input_dir", "/data/lddl", "--checkpoint_activations", "--amp", "--bf16"])
    lines = []
    hit = bp.warn_ignored_flags(a, a._defaults, log=lines.append)
    assert sorted(hit) == ["amp", "checkpoint_activations", "input_dir"] and len(lines) == 3
    assert any("--input_dir" in l and "SYNTHETIC" in l for l in lines)
    b = bp.parse_arguments(["--bf16"])
    assert bp.warn_ignored_flags(b, b._defaults, log=lines.append) == []
    for mod in (t2, wg):
        import contextlib, io
        err = io.StringIO()
        with contextlib.redirect_stderr(err):
            a = mod.parse_args(["-o", "x", "-lr", "1", "--epochs", "1", "-bs", "1", "--no-such-flag", "--local_rank", "3"])
        assert a.epochs == 1 and "--no-such-flag" in err.getvalue() and "--local_rank" in err.getvalue()
    with pytest.raises(SystemExit):                  # BERT: a misspelt flag stops the run
        import contextlib, io
        with contextlib.redirect_stderr(io.StringIO()):
            bp.parse_arguments(["--bf16", "--no-such-flag"])
