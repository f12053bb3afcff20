"""Test-set discovery for the evaluate CLI (reference: birdnet_stm32/data/dataset.py:49-99).

``load_file_paths_from_directory(root, classes, max_samples, exts)`` walks ``root/<class>/*.<ext>``,
keeps files whose parent directory is in ``classes`` (when given), caps each class at ``max_samples``
by a uniform random draw, shuffles the result with ``numpy.random`` and returns ``(paths, classes)`` —
noise-like class names ('noise', 'silence', 'background', 'other') are dropped from the class list but
their files stay.  ``os.walk`` replaces ``tf.io.gfile.walk``.
"""

from __future__ import annotations

import os

import numpy as np

SUPPORTED_AUDIO_EXTS = (".wav", ".mp3", ".flac", ".ogg", ".m4a")
_NOISE = {"noise", "silence", "background", "other"}


def load_file_paths_from_directory(directory: str, classes: list[str] | None = None, max_samples: int | None = None,
                                   exts: tuple = SUPPORTED_AUDIO_EXTS) -> tuple[list[str], list[str]]:
    by_class: dict[str, list[str]] = {}
    for root, dirs, names in os.walk(directory):
        dirs.sort()   # (directory order is the file system's: sorted, a seed gives the same shuffle, split and trained head on every machine)
        label = os.path.basename(root)
        if classes is not None and label not in classes:
            continue
        for name in sorted(names):
            if name.lower().endswith(exts):
                by_class.setdefault(label, []).append(os.path.join(root, name))
    paths: list[str] = []
    for files in by_class.values():
        if max_samples is not None and 0 < max_samples < len(files):
            files = [files[i] for i in np.random.permutation(len(files))[:max_samples]]
        paths.extend(files)
    np.random.shuffle(paths)
    return paths, sorted(c for c in by_class if c.lower() not in _NOISE)


def upsample_minority_classes(file_paths: list[str], classes: list[str], ratio: float = 0.25) -> list[str]:
    """Repeat files of the small classes until every class has ``int(largest * ratio)`` of them (reference: data/dataset.py:102-138).

    The draws are the reference's, on numpy's global generator, so ``np.random.seed(s)`` in front gives its list: per class in
    ``classes`` order that is short of the target one ``np.random.choice(paths_of_class, size=missing, replace=True)``, appended behind
    the class's own files; then one ``np.random.shuffle`` of all.  A class at or over the target is left alone, so is a class without a
    file (nothing to draw from).  As in the reference, files whose folder is no class are not in the result: ``probe`` passes the class
    files only and keeps the others itself (``training.linear_probe.upsample_multiplicity``)."""
    if not 0 < float(ratio) <= 1:
        raise ValueError(f"ratio must be in (0, 1], got {ratio}")
    members: dict[str, list[str]] = {c: [] for c in classes}
    for path in file_paths:
        label = os.path.basename(os.path.dirname(path))
        if label in members:
            members[label].append(path)
    target = int(max((len(v) for v in members.values()), default=0) * float(ratio))
    out: list[str] = []
    for c in classes:
        own = members[c]
        out.extend(own)
        if 0 < len(own) < target:
            out.extend(np.random.choice(own, size=target - len(own), replace=True).tolist())
    np.random.shuffle(out)
    return out
