#!/usr/bin/env python3
"""Generate the dataset-tool fixtures by running the REFERENCE modules in the build container
(beside tools/make_golden.py, whose cv2 / insightface stand-ins it reuses; runs only where the
reference checkout exists, never on the GPU box).

* ``tests/golden/segment_dataset.npz`` -- the reference ``segment_dataset.ProbeSegmenter`` on the
  seeded metadata list of ``tests/_dataset_cases.py`` (a few hundred entries: seeded values, values
  exactly on every threshold, blur twins, entries with keys missing), for each setting of
  ``SEGMENTER_SETTINGS`` (defaults; percentiles that push both blur indices to ``len``; another set
  of thresholds): the two blur thresholds and ``categorize_face`` of every entry; the same for a
  1-entry list; and the ten ``<category>_metadata.json`` texts of one ``segment_dataset`` run (copy
  mode) over a temporary directory in which one file's name only ends with its metadata name, one
  metadata entry has no file and one file has no metadata, with the names copied into each category.
* ``tests/golden/dataset_preprocessor.npz`` -- the reference ``DatasetPreprocessor.process_dataset``
  over the synthetic tree of ``_dataset_cases.build_tree`` (a class with angle folders, one missing; a
  flat class with ``left`` / ``right`` in file names; a class without images; a file that does not
  decode) with a stub ``processor`` that decodes the file as the reference's ``process_image`` does
  (the cv2 stand-in's ``imread``; ValueError when that fails) and answers ``_dataset_cases.faces_for``:
  the metadata JSON text and the sorted names of the crops written.

Both hold data the reference wrote, nothing of its program text.
Usage: ``python tools/make_golden_dataset.py``
"""
from __future__ import annotations

import json
import os
import sys
import tempfile

import numpy as np

TOOLS = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, TOOLS)
import make_golden as MG  # noqa: E402  (REPO on sys.path; the stand-in module texts)

sys.path.insert(0, os.path.join(MG.REPO, "tests"))
import _dataset_cases as DC  # noqa: E402


def stand_ins() -> str:
    """cv2 and insightface stand-ins of make_golden.py in a temporary directory on sys.path."""
    tmp = tempfile.mkdtemp(prefix="frgolden_ds_")
    with open(os.path.join(tmp, "cv2.py"), "w") as f:
        f.write(MG.CV2_STUB.format(repo=MG.REPO))
    for d in ("insightface", os.path.join("insightface", "utils")):
        os.makedirs(os.path.join(tmp, d), exist_ok=True)
        open(os.path.join(tmp, d, "__init__.py"), "w").close()
    with open(os.path.join(tmp, "insightface", "app.py"), "w") as f:
        f.write(MG.INSIGHTFACE_APP)
    open(os.path.join(tmp, "insightface", "utils", "face_align.py"), "w").close()
    sys.path.insert(0, tmp)
    sys.path.append(MG.REF)
    return tmp


def main() -> None:
    if not os.path.isdir(MG.REF):
        raise SystemExit("reference not present; golden files are generated in the build container only")
    tmp = stand_ins()
    import segment_dataset as ref_seg  # reference module
    import dataset_preprocessor as ref_pre  # reference module (cv2 / insightface stand-ins)
    import cv2  # the stand-in

    # ---- ProbeSegmenter
    full = DC.metadata_list()
    out = {"metadata_sha256": np.array(DC.sha_json(full)), "n": np.int32(len(full))}
    for name, kw in DC.SEGMENTER_SETTINGS.items():
        for tag, lst in (("full", full), ("one", full[41:42])):
            seg = ref_seg.ProbeSegmenter(**kw)
            with MG.quiet():
                seg.compute_blur_thresholds(lst)
            out[f"{name}__{tag}__thresholds"] = np.array([seg.blur_sharp_threshold, seg.blur_blurry_threshold],
                                                         np.float64)
            out[f"{name}__{tag}__categories"] = np.array(json.dumps([seg.categorize_face(m) for m in lst]))
    picked, files = DC.segment_run_list()
    src, meta = DC.write_segment_inputs(os.path.join(tmp, "seg"), picked, files)
    dst = os.path.join(tmp, "seg", "segmented")
    seg = ref_seg.ProbeSegmenter()
    with MG.quiet():
        seg.segment_dataset(input_dir=src, metadata_file=meta, output_dir=dst, copy_files=True)
    run = {}
    for c in seg.categories:
        with open(os.path.join(dst, c, f"{c}_metadata.json")) as f:
            text = f.read()
        run[c] = {"metadata": text, "files": sorted(n for n in os.listdir(os.path.join(dst, c))
                                                    if n != f"{c}_metadata.json")}
    out["run_sha256"] = np.array(DC.sha_json([picked, sorted(files)]))
    out["run"] = np.array(json.dumps(run))
    path = os.path.join(MG.OUT, "segment_dataset.npz")
    np.savez_compressed(path, **out)
    print("segment", len(full), "entries;", {c: len(v["files"]) for c, v in run.items()}, os.path.getsize(path), "bytes")

    # ---- DatasetPreprocessor
    class StubProcessor:  # FaceProcessor.process_image's contract (face_recognition.py:174-182)
        def process_image(self, image_path, return_all=False):
            assert return_all is True
            bgr = cv2.imread(image_path)
            if bgr is None:
                raise ValueError(f"Could not load image: {image_path}")
            return DC.faces_for(np.ascontiguousarray(bgr[..., ::-1]))

    tree = DC.build_tree(os.path.join(tmp, "classroom"))
    pre = ref_pre.DatasetPreprocessor.__new__(ref_pre.DatasetPreprocessor)  # __init__ would build FaceAnalysis
    pre.processor = StubProcessor()
    outdir = os.path.join(tmp, "preprocessed")
    import contextlib
    import io
    with MG.quiet(), contextlib.redirect_stderr(io.StringIO()):  # the reference prints a traceback per bad file
        pre.process_dataset(input_dir=tree, output_dir=outdir)
    with open(os.path.join(outdir, "probe_positive_metadata.json")) as f:
        text = f.read()
    names = sorted(os.listdir(os.path.join(outdir, "probe_positive")))
    path = os.path.join(MG.OUT, "dataset_preprocessor.npz")
    np.savez_compressed(path, tree_sha256=np.array(DC.sha_json(DC.TREE)), metadata=np.array(text),
                        files=np.array(json.dumps(names)))
    print("preprocessor", len(json.loads(text)), "faces;", names, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
