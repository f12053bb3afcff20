"""``birdnet-stm32 probe`` — train a new classifier head for your own classes on the frozen backbone (reference: ``train --linear_probe``).

``--data_path_train`` holds one folder per class (``<class>/*.wav``); folders named noise / silence / background / other are negatives.
The backbone runs once over all files (``embed``'s device path), the head is trained on the embeddings on the GPU
(``training/linear_probe.py``) and written as ``<output>.npz`` with ``<output>_labels.txt``, ``<output>_model_config.json`` and
``<output>_history.csv``.  ``analyze --head <output>.npz`` then reports those classes in recordings.  With ``--mixup_probability`` or
``--spec_augment`` the training rows' model inputs stay on the device and every epoch trains on fresh embeddings of augmented rows
(``training/augment.py``).  With ``--tune`` the learning rate, dropout, label smoothing, optimizer, weight decay and gradient clip are searched:
``--n_trials`` heads train at once on the device (``training/tune.py``), the one with the lowest validation loss is written, and
``<output>_tune.json`` lists them all.  For long-tailed folders: ``--upsample_ratio`` repeats training files of the small classes,
``--class_weights balanced`` weighs the rows by inverse class frequency and ``--loss focal`` trains on the focal loss; they combine with
each other and with the plain fit, ``--tune`` and the augmented fit.  ``--hidden_units H`` puts one ReLU layer of H units between embedding
and classes (the plain fit only).  With ``--export_tflite`` on an INT8 ``.tflite`` backbone the head is
also quantised and written into ``<output>.tflite`` (``conversion/head_export.py``), next to the labels and config: a model for
``evaluate``, ``analyze`` and the board.  ``--qat_epochs N`` then fine-tunes the head for N epochs against that quantisation first
(``training/probe_qat.py``) and writes whichever of the two heads scores better as INT8.
"""

from __future__ import annotations

import argparse


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description="Train a classifier head for new classes on the embeddings of a pretrained model.")
    p.add_argument("--model_path", type=str, required=True, help="Path to the pretrained .keras or .tflite model")
    p.add_argument("--model_config", type=str, default="", help="Path to model config JSON (default: <model>_model_config.json)")
    p.add_argument("--data_path_train", type=str, required=True, help="Directory with one folder of audio files per class")
    p.add_argument("--output", type=str, required=True, help="Output stem: writes <output>.npz, _labels.txt, _model_config.json, _history.csv")
    p.add_argument("--activation", type=str, default="sigmoid", choices=["sigmoid", "softmax"], help="sigmoid: multi-label, noise folders are negatives")
    p.add_argument("--epochs", type=int, default=50, help="Number of epochs")
    p.add_argument("--batch_size", type=int, default=32, help="Batch size (embedding rows)")
    p.add_argument("--learning_rate", type=float, default=0.001, help="Initial learning rate of the cosine schedule")
    p.add_argument("--optimizer", type=str, default="adam", choices=["adam", "adamw", "sgd"], help="Optimizer")
    p.add_argument("--weight_decay", type=float, default=0.0, help="Weight decay (adamw only)")
    p.add_argument("--grad_clip", type=float, default=1.0, help="Gradient clipping by global norm (0 to disable)")
    p.add_argument("--dropout", type=float, default=0.5, help="Dropout rate in front of the head")
    p.add_argument("--hidden_units", type=int, default=0,
                   help="Units of one ReLU layer between embedding and classes, with dropout in front of both layers; 0 = none, the linear head "
                        "(the default).  Not with --tune, --export_tflite / --qat_epochs, --mixup_probability or --spec_augment")
    p.add_argument("--label_smoothing", type=float, default=0.0,
                   help="Label smoothing of the training loss, in [0, 1); 0 = off (the default here; the reference's `train` defaults to 0.1).  "
                        "The validation loss is never smoothed")
    p.add_argument("--loss", type=str, default="auto", choices=["auto", "focal"],
                   help="auto: the activation's cross-entropy; focal: the focal loss of the sigmoid head, in training and in the validation loss "
                        "(after label smoothing, where the reference's --loss focal replaces it).  Needs --activation sigmoid")
    p.add_argument("--focal_gamma", type=float, default=2.0, help="With --loss focal: the focusing exponent, >= 0 (the reference's default)")
    p.add_argument("--class_weights", type=str, default="none", choices=["none", "balanced"],
                   help="balanced: weight every training row by total / (classes * files of its class), counted after upsampling; rows of noise "
                        "folders weigh 1; with mixup a mixed row keeps its own file's weight.  none is the default here; the reference's `train` "
                        "defaults to balanced")
    p.add_argument("--upsample_ratio", type=float, default=0.0,
                   help="Repeat training files of the small classes up to this fraction of the largest class, 0 < R <= 1 (the reference's rule "
                        "and draws); 0 = off.  Every file is still embedded once, and files of noise folders are kept once")
    p.add_argument("--val_split", type=float, default=0.2, help="Validation split ratio (by file)")
    p.add_argument("--patience", type=int, default=10, help="Early stopping: epochs without a better validation loss")
    p.add_argument("--max_duration", type=float, default=30, help="Seconds read from the start of each file")
    p.add_argument("--overlap", type=float, default=0.0, help="Chunk overlap (seconds)")
    p.add_argument("--max_chunks_per_file", type=int, default=0,
                   help="Keep only each file's N most active chunks (long files are cropped around their loudest stretches first); 0 = off, every "
                        "chunk is used.  Needs --overlap 0.  The reference's `train` defaults to 3")
    p.add_argument("--activity_threshold", type=float, default=0.1, help="With --max_chunks_per_file: drop chunks whose activity ratio is lower (one per file is always kept); validation files use 0.5, as the reference's linear probe does")
    p.add_argument("--candidate_chunks", type=int, default=0, help="With --max_chunks_per_file: chunks ranked per file (0 = min(8, max(4, 2 N)), as the reference)")
    p.add_argument("--mixup_alpha", type=float, default=0.2, help="Dirichlet concentration of the mixup gains (the reference's default)")
    p.add_argument("--mixup_probability", type=float, default=0.0,
                   help="Fraction of the training rows mixed from 2-3 rows each epoch, labels united; 0 = off (the default here; the reference's `train` "
                        "defaults to 0.25).  Needs --activation sigmoid.  The backbone then runs every epoch")
    p.add_argument("--spec_augment", action="store_true",
                   help="Mask two frequency bands and two time spans of every training row, drawn anew each epoch (off by default here; on in the "
                        "reference unless --no_spec_augment).  Spectrogram frontends only: a raw-frontend model gets no masks")
    p.add_argument("--freq_mask_max", type=int, default=8, help="With --spec_augment: widest frequency mask in bins (the reference's default)")
    p.add_argument("--time_mask_max", type=int, default=25, help="With --spec_augment: widest time mask in frames (the reference's default)")
    p.add_argument("--tune", action="store_true",
                   help="Search learning rate, dropout, label smoothing, optimizer, weight decay and gradient clip: --n_trials heads train at once, "
                        "trial 0 with this command line's own values; the head with the lowest validation loss is written (no retraining) and "
                        "<output>_tune.json lists every trial.  Needs --val_split > 0; not with --mixup_probability or --spec_augment")
    p.add_argument("--n_trials", type=int, default=20, help="With --tune: number of trials, 1..64")
    p.add_argument("--tune_seed", type=int, default=None, help="With --tune: seed of the trials' draws (default: --seed)")
    p.add_argument("--export_tflite", action="store_true",
                   help="Also write the trained head into <output>.tflite: the INT8 backbone with its classifier replaced by the quantised head, an "
                        "ordinary model for evaluate / analyze / the board, and <output>_export.json with the float-vs-INT8 report.  Needs "
                        "--model_path to be an INT8 .tflite")
    p.add_argument("--per_tensor", action="store_true", help="With --export_tflite: one weight scale for the whole head instead of one per class")
    p.add_argument("--min_cosine_sim", type=float, default=0.95,
                   help="With --export_tflite: minimum mean cosine similarity of float and INT8 head scores; the export fails below (0 to disable)")
    p.add_argument("--qat_epochs", type=int, default=0,
                   help="With --export_tflite: fine-tune the trained head for N epochs with its weights and logits quantised as the export "
                        "quantises them, then write whichever head (float-trained or fine-tuned) has the lower INT8 loss over the report rows; "
                        "0 = off.  Label smoothing and augmentation are not applied in this phase")
    p.add_argument("--qat_learning_rate", type=float, default=1e-4, help="With --qat_epochs: initial learning rate of the fine-tune (the reference's QAT default)")
    p.add_argument("--seed", type=int, default=42, help="Seed of the file shuffle, the initial weights, the batches and the dropout mask")
    p.add_argument("--max_batch", type=int, default=4096, help="Workspace size in chunks = inference slice of the device pipeline")
    p.add_argument("--device", type=int, default=0, help="MI355X index")
    return p


def main(argv=None, runner=None):
    from birdnet_stm32.training.linear_probe import run_linear_probe

    args = build_parser().parse_args(argv)
    try:
        from birdnet_stm32.audio.pipeline import selection_from_args

        selection_from_args(args)   # (bad selection flags are refused before anything is loaded, as `embed` does)
        from birdnet_stm32.training.linear_probe import augmentation_from_args, hidden_from_args, imbalance_from_args

        hidden_from_args(args)         # (--hidden_units with a path that is not built for it)
        augmentation_from_args(args)   # (and bad augmentation flags; run_linear_probe refuses bad --tune / --label_smoothing combinations first thing)
        imbalance_from_args(args)      # (and focal with softmax, a bad --focal_gamma or --upsample_ratio)
        from birdnet_stm32.training.linear_probe import check_export_args

        check_export_args(args)        # (and --export_tflite on a float backbone)
        from birdnet_stm32.training.linear_probe import check_qat_args

        check_qat_args(args)           # (and --qat_epochs without --export_tflite)
        return run_linear_probe(args, runner=runner)
    except (ValueError, FileNotFoundError) as exc:
        raise SystemExit(f"error: {exc}") from None


if __name__ == "__main__":
    main()
