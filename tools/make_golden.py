#!/usr/bin/env python3
"""Generate tests/golden/* by running the REFERENCE code in the build container.

Runs only where ``/root/reference`` exists (never on the GPU box).  It imports
the reference's own ``face_embedder.FaceEmbedder`` and
``gallery_manager.GalleryManager`` and records their outputs on seeded inputs:

* ``embed_<arch>.npz`` — reference ``extract_embeddings_batch`` (batch 32,
  face_embedder.py:137-182) on seeded gallery crops, reference
  ``extract_embedding`` (face_embedder.py:112-135) on seeded probe crops, and
  reference ``GalleryManager.search(top_k=5)`` (gallery_manager.py:189-205)
  for every probe against a gallery built with ``add_student``.
* ``c3_ir_101.npz`` — the headline configuration exactly (BASELINE.json
  configs[2]): reference IR-101 ``extract_embeddings_batch`` of the bench's
  1,000 gallery crops and 256 probe crops, a 1,000-row gallery built with the
  reference ``GalleryManager.add_student``, and reference ``search(top_k=5)``
  of every probe (gallery_manager.py:189-205).
* ``resize_ir_50.npz`` — reference ``extract_embeddings_batch`` on crops that
  are not 112x112 (224x224 enrollment crops, enroll_students.py:67-81,222, and
  odd sizes), i.e. through the ``cv2.resize`` branch of face_embedder.py:94-96.
  cv2 is absent, so for this file the stub's ``resize`` is the restatement of
  OpenCV's INTER_LINEAR in ``oracle/scrfd.py``: the fixture pins the
  reference wrapper's order of operations around it, not cv2 itself.
* ``backup_<name>.npz`` — the reference's committed gallery backups
  (``gallery/backups/*.json`` and ``backups/*.json``, export format
  gallery_manager.py:246-270) as arrays, plus reference ``GalleryManager``
  templates rebuilt by ``add_student`` and reference ``search`` results for
  every stored sample.  ``backups/adaface_ir_50_backup_20251202_081742.json``
  becomes ``backup_root_adaface_ir_50.npz``.
* ``gate.npz`` — the reference ``FaceQualityFilter.compute_pose_angles`` /
  ``is_valid`` and ``FaceProcessor.process_numpy`` (face_recognition.py:101-216)
  on the seeded frame and fixed detections of ``tests/_gate_inputs.py``, for
  three quality configurations, RGB and grayscale frames, ``return_all``
  true and false: every result's detection index, ``is_valid``, metrics
  (values and types) and aligned-crop SHA-256.  ``insightface`` is absent and
  is stubbed (``FaceAnalysis`` refuses to be built; the processor gets a
  fixed-detection detector); the cv2 calls go to the restatements in
  ``oracle/align_ref.py``, so this file pins the reference's gate logic,
  pose arithmetic, ordering and dict layout -- everything but cv2's own
  numerics.
* ``image.npz`` + ``image_{rgb,gray,rgba}.png`` — small seeded PNG files (RGB, 8-bit
  gray, RGBA) and the SHA-256 of the RGB array ``cv2.imread`` + ``COLOR_BGR2RGB`` yields
  for each (gray expanded to 3 channels, alpha dropped: IMREAD_COLOR), computed from the
  arrays the files were written from; and the reference ``FaceProcessor.process_image``
  (face_recognition.py:174-182) on the gate frame written as PNG (``imread`` in the cv2
  shim decodes through PIL: lossless, so the pixels are the frame's), with the gate's
  fixed detections, default quality settings, ``return_all`` true and false.
* ``dropin_students.pkl`` + ``dropin_students.npz`` — a gallery written by THIS repo's
  ``GalleryManager.save`` (``ref_students.pkl`` loaded, one student enrolled, one updated,
  one deleted through the drop-in), then loaded by the REFERENCE ``GalleryManager`` (the real
  ``pickle.load`` of gallery_manager.py:241-242): the records it sees (ids, names, sample
  counts, dates, array checksums) and its ``search(top_k=5)`` of every stored sample.
* ``ref_students.pkl`` / ``ref_students.json`` — the reference's own gallery
  FILES (gallery_manager.py:207-232): a reference ``GalleryManager`` built
  with ``add_student`` (samples + metadata) from
  ``gallery/backups/adaface_ir_101_backup_*.json`` and ``.save()``d.  Its
  templates and search results are those of ``backup_adaface_ir_101.npz``.
* ``track_consensus.npz`` — the reference ``FaceMatcher._aggregate_matches`` /
  ``_get_best_candidate`` (face_matcher.py:321-385), called unbound with a stand-in ``self``
  that carries only ``similarity_threshold``, on hand-built tracks (majorities, the 0.4 / 0.5
  ratio edges, ties in both orders, too few or no quality frames, the f32 neighbours of 0.55,
  tracks of 1 / 255 / 256 / 257 / 1024 frames): per group of one (k, threshold) the top-k
  ``idx`` / ``score`` / ``offsets`` a launch takes (columns past 0 are decoys) and per track the
  reference's outputs and the FR_TRACK_* status they imply; and the reference
  ``_generate_summary`` (:446-477) of all those tracks' results.

Two modules the reference imports are absent from this image and are supplied
in a temporary directory that is put on ``sys.path`` for this run only:
``net`` (upstream AdaFace, restated in ``oracle/adaface_net.py``) and ``cv2``
(only ``cv2.resize``/``INTER_LINEAR`` are referenced on the embed path; the
stub raises unless the resize restatement is switched on for the resize
fixture).  Weights are the seeded synthetic checkpoint of
``facerecognitionpipeline_amd.weights`` saved in the reference's checkpoint
format.  Crops are regenerated from their seeds at test time; their SHA-256 is
stored to pin them.

* ``capture_tracks.npz`` — the reference ``SimpleTracker`` and ``FrameAccumulator``
  (face_detection.py:11-228), driven as ``CameraFaceCapture.process_frame`` drives them (:271-283),
  on hand-built and seeded synthetic sessions (``tests/_capture_cases.py`` builds them: ties in
  both directions, the ``max_distance`` and ``max_disappeared`` edges, deletions and returns, empty
  frames, quality edges, partial tracks with and without the forced save): per session the boxes,
  metrics, validity, frame offsets and settings a launch takes, and the reference's track id,
  ``compute_quality_score`` and saved ``frame_NNN`` number of every detection and the
  ``metadata.json`` numbers of every saved track.  scipy (``cdist``) is the installed one.

* ``live_tracks.npz`` — the reference ``LiveFaceRecognition.process_frame`` (face_recognition_live.py:
  320-414) with its ``LiveRecognitionTracker``, ``_update_attendance`` and ``_finalize_session``, on the
  hand-built and seeded sessions of ``tests/_live_cases.py``.  The object is built without its
  constructor (which loads models); its processor replays the session's detections, its embedder
  returns the prepared unit vector of the crop it is handed, its gallery is the reference
  ``GalleryManager`` over basis-vector templates.  ``performance_monitor_server`` is supplied as a
  stub: the reference imports a ``PerformanceMonitor`` name that module does not define, and
  monitoring is off.  Per session: the boxes, metrics, frame offsets, plans and settings, and the
  reference's track id of every detection, its attempt log (tick detection, track, attempt number,
  best detection, top-3 students and scores), ``attendance.json`` without its clock and folder
  fields, and the statistics of ``session.json``.

* ``evaluate.npz`` — the evaluation functions of ``evaluate_models_v2.ipynb`` (``cosine_similarity``,
  ``compute_all_similarities``, ``aggregate_*``, ``identify_probe``, ``compute_rank_metrics``,
  ``compute_dprime``, ``bootstrap_confidence_interval`` and the four ``evaluate_*_comprehensive``).  The
  notebook is read as JSON at run time and only the code cells that define those functions are
  executed (``tqdm`` is the identity; pandas and sklearn are the installed ones); none of its text is
  written anywhere.  They run on the cases of ``tests/_eval_cases.py`` (``exact``: basis-vector
  galleries and hand-built score lists; ``seeded``: 13 identities of 1..1024 rows, segments and
  negatives; ``norms``: off-unit rows): per case and (aggregation, k) the reference's similarity and
  identity-score matrices, predictions, ranks, every threshold table, the per-identity table and the
  verification figures, as arrays; the inputs are pinned by SHA-256.  The builder asserts the
  margins of ``_eval_cases.check_margins`` on the reference's numbers, that the host statements of
  ``facerecognitionpipeline_amd.evaluate_models`` reproduce the reference bit for bit on ``exact``,
  and that ``eval_probes_host`` reproduces its records and counts on every recorded score matrix.

Usage: ``python tools/make_golden.py [embed] [c3] [resize] [backups] [refpkl] [gate] [image] [track] [capture] [live] [evaluate] [dropin]``
(no argument: all).
"""
from __future__ import annotations

import contextlib
import glob
import hashlib
import io
import json
import os
import sys
import tempfile

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference"
OUT = os.path.join(REPO, "tests", "golden")
sys.path.insert(0, REPO)

from facerecognitionpipeline_amd import weights as W  # noqa: E402

N_GALLERY = 8
N_PROBE = 8
TOP_K = 5

C3_GALLERY = 1000   # BASELINE.json configs[2]: gallery=1k, batch=256, top-5
C3_PROBES = 256
RESIZE_SIZES = ((224, 224),) * 6 + ((150, 130), (96, 96))   # (H, W) of the resize-branch crops
RESIZE_SEED = 0xFACE0224

CV2_STUB = '''import sys
INTER_LINEAR = 1
RESTATED_RESIZE = False
def resize(img, dsize, interpolation=INTER_LINEAR):
    if not RESTATED_RESIZE:
        raise RuntimeError("cv2 stub: resize is not expected on the 112x112 golden path")
    sys.path.insert(0, {repo!r})
    from oracle.scrfd import resize_linear_u8  # restatement of cv::resize INTER_LINEAR (uint8)
    assert interpolation == INTER_LINEAR
    return resize_linear_u8(img, int(dsize[0]), int(dsize[1]))

# face_recognition.py's calls (gate fixture): delegated to the restatements in oracle/align_ref.py
COLOR_RGB2BGR = COLOR_BGR2RGB = 4
COLOR_RGB2GRAY = 7
COLOR_GRAY2BGR = 8
CV_64F = 6
BORDER_CONSTANT = 0
def _A():
    sys.path.insert(0, {repo!r})
    from oracle import align_ref
    return align_ref
def cvtColor(img, code):
    import numpy as np
    if code == COLOR_RGB2BGR:
        return np.ascontiguousarray(img[..., ::-1])
    if code == COLOR_GRAY2BGR:
        return np.repeat(img[..., None], 3, axis=2)
    if code == COLOR_RGB2GRAY:
        return _A().rgb_to_gray(img)
    raise NotImplementedError(code)
def estimateAffinePartial2D(src, dst):
    return _A().fit_similarity(src, dst), None
def getAffineTransform(src, dst):
    raise NotImplementedError("not on the similarity path")
def warpAffine(img, M, dsize, flags=INTER_LINEAR, borderMode=BORDER_CONSTANT, borderValue=0):
    assert flags == INTER_LINEAR and borderMode == BORDER_CONSTANT and borderValue == 0 and dsize[0] == dsize[1]
    if img.ndim == 2:
        return _A().warp_affine_linear(img[:, :, None], M, int(dsize[0]))[:, :, 0]
    return _A().warp_affine_linear(img, M, int(dsize[0]))
def imread(path, flags=1):
    # IMREAD_COLOR of an 8-bit file: 3-channel BGR, or None when unreadable; decoded by PIL
    # (lossless formats decode to the same bytes; this pins process_image's wrapper, not imread)
    import numpy as np
    try:
        from PIL import Image
        with Image.open(path) as im:
            im.load()
            return np.ascontiguousarray(np.asarray(im.convert("RGB"), dtype=np.uint8)[..., ::-1])
    except (OSError, ValueError, SyntaxError):
        return None
def imwrite(path, img):
    # face_detection.py's save_track (capture fixture): BGR in, written through PIL (bytes unpinned)
    import numpy as np
    from PIL import Image
    Image.fromarray(np.ascontiguousarray(img[..., ::-1])).save(path, quality=95)
    return True
def Laplacian(gray, ddepth):
    import numpy as np
    assert ddepth == CV_64F
    g = gray.astype(np.float64)
    p = np.pad(g, 1, mode="reflect")  # BORDER_REFLECT_101, ksize 1: [0 1 0; 1 -4 1; 0 1 0]
    return p[:-2, 1:-1] + p[2:, 1:-1] + p[1:-1, :-2] + p[1:-1, 2:] - 4.0 * g
'''
# insightface is absent: FaceAnalysis('buffalo_l') would download its model pack, so the stub
# refuses to be constructed; FaceProcessor gets a fixed-detection stub detector instead
INSIGHTFACE_APP = '''class FaceAnalysis:
    def __init__(self, *a, **k):
        raise RuntimeError("insightface stub: FaceAnalysis is never constructed for the golden files")
'''
NET_SHIM = '''import sys
sys.path.insert(0, {repo!r})
from oracle.adaface_net import build_model  # restated upstream AdaFace net.py
'''


def sha(a: np.ndarray) -> str:
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def quiet():
    return contextlib.redirect_stdout(io.StringIO())


def main() -> None:
    if not os.path.isdir(REF):
        raise SystemExit("reference not present; golden files are generated in the build container only")
    parts = set(sys.argv[1:]) or {"embed", "c3", "resize", "backups", "refpkl", "gate", "image", "track",
                                     "capture", "live", "evaluate", "dropin"}
    os.makedirs(OUT, exist_ok=True)
    tmp = tempfile.mkdtemp(prefix="frgolden_")
    with open(os.path.join(tmp, "cv2.py"), "w") as f:
        f.write(CV2_STUB.format(repo=REPO))
    with open(os.path.join(tmp, "net.py"), "w") as f:
        f.write(NET_SHIM.format(repo=REPO))
    for d in ("insightface", os.path.join("insightface", "utils")):
        os.makedirs(os.path.join(tmp, d), exist_ok=True)
        open(os.path.join(tmp, d, "__init__.py"), "w").close()
    with open(os.path.join(tmp, "insightface", "app.py"), "w") as f:
        f.write(INSIGHTFACE_APP)
    open(os.path.join(tmp, "insightface", "utils", "face_align.py"), "w").close()
    sys.path.insert(0, tmp)
    sys.path.append(REF)
    import torch
    torch.set_num_threads(min(8, os.cpu_count() or 1))
    import face_embedder as ref_fe  # reference module
    import gallery_manager as ref_gm  # reference module

    def embedder(arch):
        ckpt = os.path.join(tmp, f"{arch}.ckpt")
        if not os.path.exists(ckpt):
            W.save_checkpoint(W.synthetic_state_dict(arch), ckpt)
        with quiet():
            return ref_fe.FaceEmbedder(architecture=arch, model_path=ckpt, model_type="adaface",
                                       device=torch.device("cpu"))

    def search_arrays(gm, queries):
        with quiet():
            res = [gm.search(q, top_k=TOP_K) for q in queries]
            gal, ids = gm.get_gallery_embeddings()
        pos = {sid: i for i, sid in enumerate(ids)}
        idx = np.array([[pos[sid] for sid, _n, _s in r] for r in res], dtype=np.int32)
        sc = np.array([[s for _sid, _n, s in r] for r in res], dtype=np.float32)
        return gal, idx, sc

    if "embed" in parts:
        base = W.synthetic_crops(N_GALLERY, W.CROP_SEED_GALLERY)
        probes = W.probe_crops(base, N_PROBE)
        for arch in ("ir_50", "ir_101"):
            emb = embedder(arch)
            with quiet():
                g = emb.extract_embeddings_batch(list(base), normalize=True, batch_size=32)
                p = np.stack([emb.extract_embedding(x, normalize=True) for x in probes])
                gm = ref_gm.GalleryManager(gallery_path=os.path.join(tmp, f"g_{arch}", "students.pkl"))
                for i in range(N_GALLERY):
                    gm.add_student(f"S{i:03d}", f"N{i}", g[i])
            gal, ids_arr, sc_arr = search_arrays(gm, p)
            np.savez_compressed(
                os.path.join(OUT, f"embed_{arch}.npz"),
                weight_seed=np.int64(W.DEFAULT_WEIGHT_SEED), gallery_seed=np.int64(W.CROP_SEED_GALLERY),
                probe_seed=np.int64(W.CROP_SEED_PROBE),
                gallery_crops_sha256=np.array(sha(base)), probe_crops_sha256=np.array(sha(probes)),
                gallery_emb=g.astype(np.float32), probe_emb=p.astype(np.float32),
                gallery_matrix=gal.astype(np.float32),
                search_idx=ids_arr, search_score=sc_arr)
            print(arch, "gallery", g.shape, "probe", p.shape, "top1", ids_arr[:, 0].tolist())

    if "c3" in parts:
        # exactly the bench workload (bench.py: W.synthetic_crops(1000, CROP_SEED_GALLERY) and rank 0's
        # W.probe_crops(gal, 256, seed=CROP_SEED_PROBE)); every probe through the reference embedder,
        # every gallery row through add_student, every search through the reference search
        gal_crops = W.synthetic_crops(C3_GALLERY, W.CROP_SEED_GALLERY)
        probes = W.probe_crops(gal_crops, C3_PROBES, seed=W.CROP_SEED_PROBE)
        emb = embedder("ir_101")
        with quiet():
            g = emb.extract_embeddings_batch(list(gal_crops), normalize=True, batch_size=32)
            p = emb.extract_embeddings_batch(list(probes), normalize=True, batch_size=32)
            gm = ref_gm.GalleryManager(gallery_path=os.path.join(tmp, "c3", "students.pkl"))
            for i in range(C3_GALLERY):
                gm.add_student(f"S{i:04d}", f"N{i}", g[i])
        gal, ids_arr, sc_arr = search_arrays(gm, p)
        # single-sample add_student keeps the row as is (gallery_manager.py:298-299): the reference
        # gallery matrix IS the embedding matrix, stored once
        assert np.array_equal(gal, g)
        np.savez_compressed(
            os.path.join(OUT, "c3_ir_101.npz"),
            weight_seed=np.int64(W.DEFAULT_WEIGHT_SEED), gallery_seed=np.int64(W.CROP_SEED_GALLERY),
            probe_seed=np.int64(W.CROP_SEED_PROBE),
            gallery_crops_sha256=np.array(sha(gal_crops)), probe_crops_sha256=np.array(sha(probes)),
            gallery_emb=g.astype(np.float32), probe_emb=p.astype(np.float32),
            search_idx=ids_arr, search_score=sc_arr)
        print("c3", g.shape, p.shape, "top1 == i mod G:", float((ids_arr[:, 0] == np.arange(C3_PROBES) % C3_GALLERY).mean()))

    if "resize" in parts:
        import cv2  # the stub above
        cv2.RESTATED_RESIZE = True
        r = np.random.Generator(np.random.PCG64(RESIZE_SEED))
        crops = [r.integers(0, 256, size=(h, w, 3), dtype=np.uint8) for h, w in RESIZE_SIZES]
        emb = embedder("ir_50")
        with quiet():
            e = emb.extract_embeddings_batch(crops, normalize=True, batch_size=32)
        cv2.RESTATED_RESIZE = False
        np.savez_compressed(
            os.path.join(OUT, "resize_ir_50.npz"), weight_seed=np.int64(W.DEFAULT_WEIGHT_SEED),
            crop_seed=np.int64(RESIZE_SEED), sizes=np.array(RESIZE_SIZES, dtype=np.int32),
            crops_sha256=np.array(sha(np.concatenate([c.ravel() for c in crops]))), emb=e.astype(np.float32))
        print("resize", e.shape)

    if "backups" in parts:
        paths = sorted(glob.glob(os.path.join(REF, "gallery", "backups", "*.json")))
        paths += sorted(glob.glob(os.path.join(REF, "backups", "*.json")))
        for path in paths:
            name = os.path.basename(path).split("_backup_")[0]
            if os.path.dirname(path) == os.path.join(REF, "backups"):
                name = "root_" + name
            with open(path) as f:
                data = json.load(f)
            sids = list(data["students"].keys())
            emb = np.array([data["students"][s]["embeddings"] for s in sids], dtype=np.float32)
            tmpl = np.array([data["students"][s]["template_embedding"] for s in sids], dtype=np.float32)
            avg = np.array([data["students"][s]["metadata"].get("avg_similarity", np.nan) for s in sids],
                           dtype=np.float64)
            with quiet():
                gm = ref_gm.GalleryManager(gallery_path=os.path.join(tmp, f"b_{name}", "students.pkl"),
                                           aggregation_method="mean")
                for s in sids:
                    gm.add_student(s, data["students"][s]["name"], np.array(data["students"][s]["embeddings"],
                                                                             dtype=np.float32))
            gal, idx, sc = search_arrays(gm, emb.reshape(-1, emb.shape[-1]))
            np.savez_compressed(
                os.path.join(OUT, f"backup_{name}.npz"),
                student_ids=np.array(sids), embeddings=emb, stored_template=tmpl, avg_similarity=avg,
                ref_template=gal.astype(np.float32), search_idx=idx, search_score=sc)
            print(name, emb.shape)

    if "refpkl" in parts:
        import shutil
        path = sorted(glob.glob(os.path.join(REF, "gallery", "backups", "adaface_ir_101_backup_*.json")))[0]
        with open(path) as f:
            data = json.load(f)
        d = os.path.join(tmp, "refpkl")
        with quiet():
            gm = ref_gm.GalleryManager(gallery_path=os.path.join(d, "students.pkl"), aggregation_method="mean")
            for sid, rec in data["students"].items():
                gm.add_student(sid, rec["name"], np.array(rec["embeddings"], dtype=np.float32),
                               metadata=rec.get("metadata") or {})
            gm.save()
        shutil.copyfile(os.path.join(d, "students.pkl"), os.path.join(OUT, "ref_students.pkl"))
        shutil.copyfile(os.path.join(d, "students.json"), os.path.join(OUT, "ref_students.json"))
        print("refpkl", len(data["students"]), "students from", os.path.basename(path))

    if "gate" in parts:
        import face_recognition as ref_fr  # reference module (insightface / cv2 stubbed above)
        sys.path.insert(0, os.path.join(REPO, "tests"))
        import _gate_inputs as GI
        frame = GI.frame()
        dets = GI.detections()

        class FixedDetector:  # the reference detector's output contract (face_recognition.py:37-48)
            def detect(self, image):
                return [{"bbox": d["bbox"].copy(), "landmarks": d["landmarks"].copy(), "det_score": d["det_score"],
                         "pose": None, "age": None, "gender": None} for d in dets]

        def enc(v):
            return {"v": float(v), "t": type(v).__name__}

        records = []
        for ci, cfg in enumerate(GI.QUALITY_CONFIGS):
            qf = ref_fr.FaceQualityFilter(**cfg)
            al = ref_fr.FaceAligner(output_size=GI.S)
            fp = ref_fr.FaceProcessor.__new__(ref_fr.FaceProcessor)  # __init__ would build FaceAnalysis
            fp.detector, fp.aligner, fp.quality_filter = FixedDetector(), al, qf
            for kind, img in (("rgb", frame), ("gray", GI.frame_gray(frame))):
                with quiet():
                    per_face = []
                    for d in dets:
                        crop = al.align(img, d["landmarks"])
                        ok, m = qf.is_valid(d, crop)
                        per_face.append({"is_valid": bool(ok), "metrics": {k: enc(v) for k, v in m.items()},
                                         "pose": {k: enc(v) for k, v in qf.compute_pose_angles(d["landmarks"]).items()},
                                         "crop_sha256": sha(crop)})
                    runs = {}
                    for ra in (False, True):
                        res = fp.process_numpy(img, return_all=ra)
                        runs[str(ra)] = [{"det": next(i for i, d in enumerate(dets)
                                                      if np.array_equal(d["landmarks"], r["landmarks"])),
                                          "is_valid": bool(r["is_valid"]), "det_score": r["det_score"],
                                          "metrics": {k: enc(v) for k, v in r["quality_metrics"].items()},
                                          "crop_sha256": sha(r["aligned_face"]), "crop_ndim": int(r["aligned_face"].ndim),
                                          "keys": sorted(r)} for r in res]
                records.append({"config": ci, "frame": kind, "per_face": per_face, "process_numpy": runs})
        np.savez_compressed(os.path.join(OUT, "gate.npz"), frame_sha256=np.array(sha(frame)),
                            records=np.array(json.dumps(records)))
        valid = sum(f["is_valid"] for r in records for f in r["per_face"])
        print("gate", len(records), "runs,", valid, "valid of", sum(len(r["per_face"]) for r in records))

    if "image" in parts:
        from PIL import Image
        import face_recognition as ref_fr  # reference module (insightface / cv2 stubbed above)
        sys.path.insert(0, os.path.join(REPO, "tests"))
        import _gate_inputs as GI
        r = np.random.Generator(np.random.PCG64(0xFACE0B4D))
        rgb = r.integers(0, 256, (48, 64, 3), dtype=np.uint8)
        gray = r.integers(0, 256, (48, 64), dtype=np.uint8)
        rgba = r.integers(0, 256, (48, 64, 4), dtype=np.uint8)
        Image.fromarray(rgb, "RGB").save(os.path.join(OUT, "image_rgb.png"))
        Image.fromarray(gray, "L").save(os.path.join(OUT, "image_gray.png"))
        Image.fromarray(rgba, "RGBA").save(os.path.join(OUT, "image_rgba.png"))
        want = {"image_rgb.png": sha(rgb), "image_gray.png": sha(np.repeat(gray[:, :, None], 3, axis=2)),
                "image_rgba.png": sha(rgba[..., :3])}
        frame = GI.frame()
        dets = GI.detections()

        class FixedDetector2:
            def detect(self, image):
                assert np.array_equal(image, frame)  # process_image handed process_numpy the RGB frame
                return [{"bbox": d["bbox"].copy(), "landmarks": d["landmarks"].copy(), "det_score": d["det_score"],
                         "pose": None, "age": None, "gender": None} for d in dets]

        png = os.path.join(tmp, "gate_frame.png")
        Image.fromarray(frame, "RGB").save(png)
        fp = ref_fr.FaceProcessor.__new__(ref_fr.FaceProcessor)
        fp.detector, fp.aligner, fp.quality_filter = (FixedDetector2(), ref_fr.FaceAligner(output_size=GI.S),
                                                      ref_fr.FaceQualityFilter())
        runs = {}
        with quiet():
            for ra in (False, True):
                res = fp.process_image(png, return_all=ra)
                runs[str(ra)] = [{"det": next(i for i, d in enumerate(dets)
                                              if np.array_equal(d["landmarks"], r["landmarks"])),
                                  "is_valid": bool(r["is_valid"]), "crop_sha256": sha(r["aligned_face"]),
                                  "blur": float(r["quality_metrics"].get("blur_score", -1.0))} for r in res]
            try:
                fp.process_image(os.path.join(tmp, "missing.png"))
                missing = None
            except ValueError as e:
                missing = str(e).replace(tmp, "<dir>")
        np.savez_compressed(os.path.join(OUT, "image.npz"), decoded_sha256=np.array(json.dumps(want)),
                            process_image=np.array(json.dumps(runs)), missing_error=np.array(missing))
        print("image", {k: len(v) for k, v in runs.items()}, missing)

    if "track" in parts:
        import types
        import face_matcher as ref_fm  # reference module (cv2 / net stubbed above)
        A, B, C, D, E, F = 99999, 7, 31337, 0, 512, 65536  # gallery rows; A: the last row of a 100k gallery
        f32 = np.float32
        below = np.nextafter(f32(0.55), f32(0))  # the f32 just under f32(0.55)
        assert float(f32(0.55)) >= 0.55 > float(below)
        q = [0.80, 0.70, 0.75, 0.60, 0.66, 0.91, 0.58, 0.62, 0.73, 0.69, 0.77]
        R, FEW, NOC, BEL = 0, 1, 2, 3  # FR_TRACK_* as the issue states them per case
        # (label, k, similarity_threshold, rows, scores, status)
        cases = [
            ("01_majority", 1, 0.5, [A, A, A, B], q[:4], R),
            ("02_5_2_1_1_1_1", 3, 0.5, [A, B, A, C, A, D, B, A, E, F, A], q[:11], R),
            ("03_4_2_1_1_1_1_ratio_0.4", 1, 0.5, [A, B, A, C, A, D, B, A, E, F], q[:10], NOC),
            ("04_2_1_1_second_rule", 3, 0.5, [A, B, A, C], q[:4], R),
            ("05_tie_aabb", 1, 0.5, [A, A, B, B], q[:4], NOC),
            ("05_tie_baab", 3, 0.5, [B, A, A, B], q[:4], NOC),
            ("06_3_2_ratio_0.6", 1, 0.5, [B, A, B, A, B], q[:5], R),
            ("07_three_quality_frames", 3, 0.5, [B, A, A, B, A, B], [0.30, 0.60, 0.70, 0.20, 0.65, 0.54], R),
            ("08_two_quality_frames", 1, 0.5, [B, A, B, A, B], [0.50, 0.70, 0.40, 0.60, 0.30], FEW),
            ("09_no_quality_frames", 3, 0.5, [B, A, B, A, B, C], [-0.10, 1e-30, 0.30, 0.54, 1e-8, -0.999], FEW),
            ("10_below_threshold", 3, 0.6, [A, A, B, A, A], [0.56, 0.57, 0.90, 0.58, 0.57], BEL),
            ("11_edge_quality", 1, 0.5, [A, A, A], [f32(0.55)] * 3, R),
            ("11_edge_below", 1, 0.5, [A, A, A], [f32(0.55), f32(0.55), below], FEW),
        ]
        r = np.random.Generator(np.random.PCG64(0xFACE07AC))
        for n in (1, 255, 256, 257, 1024):  # block-stride sizes: seeded rows of 3 ids, scores about 0.55
            p = [0.45, 0.35, 0.2] if n in (255, 256) else [0.6, 0.25, 0.15]
            cases.append((f"12_len_{n}", 1 if n % 2 else 3, 0.5, r.choice([A, B, C], size=n, p=p).tolist(),
                          r.uniform(0.45, 0.95, size=n).astype(f32).tolist(), None))

        def stand_in(thr):  # the two vote functions read nothing of self but the threshold
            return types.SimpleNamespace(similarity_threshold=thr)

        def frame_matches(rows, scores):
            return [{"frame": f"{i:06d}.jpg", "student_id": f"S{row:06d}", "name": f"N{row}", "score": float(f32(s))}
                    for i, (row, s) in enumerate(zip(rows, scores))]

        groups = sorted({(k, thr) for _l, k, thr, _r, _s, _st in cases})
        out = {"labels": np.array([c[0] for c in cases]), "n_groups": np.int32(len(groups)),
               "min_quality": np.float64(0.55), "min_frames": np.int32(3)}
        results = []  # match_track-shaped results of every track, for _generate_summary
        for g, (k, thr) in enumerate(groups):
            mine = [c for c in cases if (c[1], c[2]) == (k, thr)]
            total = sum(len(c[3]) for c in mine)
            idx = np.zeros((total, k), np.int32)
            score = np.zeros((total, k), f32)
            rec = {n: [] for n in ("agg_none", "status", "row", "confidence", "consensus_strength",
                                   "num_quality_frames", "total_frames_evaluated", "cand_row", "cand_confidence",
                                   "cand_num_quality_frames")}
            at = 0
            offsets = [0]
            for label, _k, _thr, rows, scores, want in mine:
                n = len(rows)
                idx[at:at + n, 0] = rows
                score[at:at + n, 0] = np.asarray(scores, f32)
                for c in range(1, k):  # decoys in the other columns: a vote that read them would differ
                    idx[at:at + n, c] = (np.asarray(rows) + 13 * c) % 100000
                    score[at:at + n, c] = score[at:at + n, 0] * f32(1.0 - 0.05 * c)
                at += n
                offsets.append(at)
                fm = frame_matches(rows, scores)
                with quiet():
                    agg = ref_fm.FaceMatcher._aggregate_matches(stand_in(thr), fm, {})
                    cand = ref_fm.FaceMatcher._get_best_candidate(stand_in(thr), fm, {})
                    loose = ref_fm.FaceMatcher._aggregate_matches(stand_in(-np.inf), fm, {})
                nq = sum(m["score"] >= 0.55 for m in fm)
                status = R if agg is not None else BEL if loose is not None else FEW if nq < 3 else NOC
                assert want is None or status == want, (label, status, want)
                rec["agg_none"].append(agg is None)
                rec["status"].append(status)
                rec["row"].append(int(agg["student_id"][1:]) if agg else -1)
                rec["confidence"].append(agg["confidence"] if agg else np.nan)
                rec["consensus_strength"].append(agg["consensus_strength"] if agg else np.nan)
                rec["num_quality_frames"].append(agg["num_quality_frames"] if agg else -1)
                rec["total_frames_evaluated"].append(agg["total_frames_evaluated"] if agg else -1)
                rec["cand_row"].append(int(cand["student_id"][1:]))
                rec["cand_confidence"].append(cand["confidence"])
                rec["cand_num_quality_frames"].append(cand["num_quality_frames"])
                if agg is not None:
                    results.append({"track_id": label, "recognized": True, "student_id": agg["student_id"],
                                    "name": agg["name"], "confidence": agg["confidence"]})
                else:
                    results.append({"track_id": label, "recognized": False, "reason": "below_threshold",
                                    "best_candidate": cand})
                print("track", label, "k", k, "thr", thr, "status", status, "cand", cand["student_id"],
                      cand["confidence"])
            out[f"g{g}_labels"] = np.array([c[0] for c in mine])
            out[f"g{g}_k"] = np.int32(k)
            out[f"g{g}_similarity_threshold"] = np.float64(thr)
            out[f"g{g}_idx"], out[f"g{g}_score"] = idx, score
            out[f"g{g}_offsets"] = np.asarray(offsets, np.int32)
            for name, v in rec.items():
                out[f"g{g}_{name}"] = np.asarray(v)
        n_rec = sum(x["recognized"] for x in results)
        me = types.SimpleNamespace(similarity_threshold=0.5, aggregation_method="consensus")
        summary = ref_fm.FaceMatcher._generate_summary(me, results, n_rec, len(results) - n_rec)
        empty = ref_fm.FaceMatcher._generate_summary(me, [], 0, 0)
        out["summary_results"] = np.array(json.dumps(results))
        out["summary_ref"] = np.array(json.dumps(summary))
        out["summary_ref_empty"] = np.array(json.dumps(empty))
        np.savez_compressed(os.path.join(OUT, "track_consensus.npz"), **out)
        print("track", len(cases), "tracks in", len(groups), "groups;", n_rec, "recognized")

    if "capture" in parts:
        import face_detection as ref_fd  # reference module (cv2 / insightface stubbed above; scipy is real)
        sys.path.insert(0, os.path.join(REPO, "tests"))
        import _capture_cases as CC
        from facerecognitionpipeline_amd.face_detection import capture_tracks_host

        def ref_quality(m):
            acc = ref_fd.FrameAccumulator.__new__(ref_fd.FrameAccumulator)  # compute_quality_score reads no state
            return acc.compute_quality_score({"det_score": float(m[0]), "quality_metrics": {
                "blur_score": float(m[1]), "yaw": float(m[2]), "pitch": float(m[3]), "roll": float(m[4])}})

        edge = ref_quality(CC.EDGE)
        assert type(edge) is float, type(edge)
        built = CC.build_sessions(edge)
        out = {"n_sessions": np.int32(len(built))}
        reached = set()
        for s, sess in enumerate(built):
            bbox, metrics, valid, offsets = CC.arrays(sess)
            assert 12 <= len(offsets) - 1 <= 40 and max(np.diff(offsets)) <= 8, (s, len(offsets) - 1)
            d = {"bbox": bbox, "metrics": metrics, "valid": valid, "frame_offsets": offsets}
            tracker = ref_fd.SimpleTracker(max_disappeared=sess["max_disappeared"], max_distance=sess["max_distance"])
            with quiet():
                acc = ref_fd.FrameAccumulator(target_frames=sess["target_frames"],
                                              min_quality_score=sess["min_quality_score"],
                                              output_dir=os.path.join(tmp, f"capture_{s}"))
                ids = CC.drive(tracker, acc, d, bool(sess["save_partial"]))
            quality = np.array([ref_quality(m) for m in metrics], dtype=np.float64)
            slot = CC.saved_slots(acc, len(valid))
            meta = [acc.metadata[t] for t in sorted(acc.metadata)]
            for m in meta:  # the folder the reference wrote
                track_dir = os.path.join(tmp, f"capture_{s}", f"track_{m['track_id']:03d}")
                assert sorted(os.listdir(track_dir)) == m["files"] + ["metadata.json"], track_dir
            trace = set()
            params = {k: sess[k] for k in CC.PARAMS}
            h_ids, h_quality, h_slot, h_info = capture_tracks_host(bbox, metrics, valid, offsets, trace=trace, **params)
            # the host statement of the kernel's contract is the reference, or the fixture is not written
            assert np.array_equal(h_ids, ids) and np.array_equal(h_slot, slot), s
            assert h_quality.tobytes() == quality.tobytes(), s
            assert h_info == [tracker.next_track_id - 1, sum(m["num_frames"] == sess["target_frames"] for m in meta),
                              int((slot >= 0).sum()), 0], (s, h_info)
            reached |= trace
            for name, v in (("track_id", ids), ("quality", quality), ("slot", slot),
                            ("n_tracks", np.int32(tracker.next_track_id - 1)),
                            ("meta_track_id", np.array([m["track_id"] for m in meta], np.int32)),
                            ("meta_num_frames", np.array([m["num_frames"] for m in meta], np.int32)),
                            ("meta_avg_quality", np.array([m["avg_quality"] for m in meta], np.float64)),
                            ("meta_avg_det_score", np.array([m["avg_det_score"] for m in meta], np.float64)),
                            ("max_disappeared", np.int32(sess["max_disappeared"])),
                            ("max_distance", np.float64(sess["max_distance"])),
                            ("target_frames", np.int32(sess["target_frames"])),
                            ("min_quality_score", np.float64(sess["min_quality_score"])),
                            ("save_partial", np.int32(sess["save_partial"]))):
                d[name] = v
            for name, v in d.items():
                out[f"s{s}_{name}"] = v
            print("capture session", s, "frames", len(offsets) - 1, "detections", len(valid), "tracks",
                  tracker.next_track_id - 1, "saved", sorted(acc.metadata), sorted(trace))
        assert reached >= CC.REQUIRED, sorted(CC.REQUIRED - reached)
        np.savez_compressed(os.path.join(OUT, "capture_tracks.npz"), **out)
        print("capture", len(built), "sessions;", os.path.getsize(os.path.join(OUT, "capture_tracks.npz")), "bytes")

    if "live" in parts:
        import functools
        from datetime import datetime
        with open(os.path.join(tmp, "performance_monitor_server.py"), "w") as f:
            f.write("class PerformanceMonitor:\n    def __init__(self, *a, **k):\n"
                    "        raise RuntimeError('stub: monitoring is off for the golden files')\n")
        import face_recognition_live as ref_live  # reference module
        import tests._live_cases as LC
        from facerecognitionpipeline_amd import face_recognition_live as ours

        gallery_dir = os.path.join(tmp, "live_gallery")
        with quiet():
            gm = ref_gm.GalleryManager(gallery_path=os.path.join(gallery_dir, "students.pkl"))
            for sid, name, t in zip(LC.STUDENT_IDS, LC.STUDENT_NAMES, LC.templates()):
                gm.add_student(sid, name, t)
        host_gallery = LC.HostGallery()
        built = LC.build_sessions()
        out = {"n_sessions": np.int32(len(built))}
        reached = set()
        for s, sess in enumerate(built):
            bbox, metrics, offsets, plan_student, plan_score = LC.arrays(sess)
            assert 12 <= len(offsets) - 1 <= 40 and max(np.diff(offsets)) <= 8, (s, len(offsets) - 1)
            d = {"bbox": bbox, "metrics": metrics, "frame_offsets": offsets, "plan_student": plan_student,
                 "plan_score": plan_score}
            live = ref_live.LiveFaceRecognition.__new__(ref_live.LiveFaceRecognition)
            live.similarity_threshold = sess["similarity_threshold"]
            live.recognition_interval = sess["recognition_interval"]
            live.max_recognition_attempts = sess["max_attempts"]
            live.face_processor = LC.ReplayProcessor(d)
            live.embedder = LC.PlanEmbedder(d)
            live.gallery = gm
            live.session_name = f"live_{s}"
            live.session_dir = os.path.join(tmp, "live_sessions", live.session_name)
            live.perf_monitor = None
            live.tracker = ref_live.LiveRecognitionTracker(recognition_interval=sess["recognition_interval"],
                                                           max_attempts=sess["max_attempts"],
                                                           buffer_size=sess["buffer_size"])
            live.recognized_faces_dir = os.path.join(live.session_dir, "recognized_faces")
            live.unrecognized_faces_dir = os.path.join(live.session_dir, "unrecognized_faces")
            os.makedirs(live.recognized_faces_dir)
            os.makedirs(live.unrecognized_faces_dir)
            live.auto_snapshot = False
            live.session_start = datetime.now()
            live.frame_count = live.total_faces_detected = live.total_recognition_attempts = 0
            live.active_tracks, live.next_track_id = {}, 0
            # max_distance is a default argument of _simple_track_assignment, which process_frame leaves alone
            live._simple_track_assignment = functools.partial(live._simple_track_assignment,
                                                              max_distance=sess["max_distance"])
            with quiet():
                live._init_session_files()
                ids, log = LC.drive(live, d)
                live._finalize_session()
            assert all(e[4] is not None for e in log), s
            rows, top_idx, top_score = LC.log_arrays(log)
            with open(os.path.join(live.session_dir, "attendance.json")) as f:
                attendance = LC.strip(json.load(f))
            with open(os.path.join(live.session_dir, "session.json")) as f:
                statistics = json.load(f)["statistics"]
            statistics.pop("average_fps")
            assert statistics["total_recognition_attempts"] == len(log), s
            # the host statement of the kernel's contract is the reference, or the fixture is not written
            trace = set()
            kernel = {k: sess[k] for k in LC.SETTINGS if k != "similarity_threshold"}
            h_ids, h_prev, h_attempt, h_best, h_info = ours.live_tracks_host(bbox, metrics, offsets, trace=trace, **kernel)
            assert np.array_equal(h_ids, ids), s
            h_log, h_events = ours.resolve_attempts(h_ids.tolist(), h_attempt, h_best, LC.recognise_with(d, host_gallery),
                                                    sess["similarity_threshold"], sess["max_attempts"], trace=trace)
            assert [(e["det"], e["track"], e["attempt"], e["best"]) for e in h_log] == [tuple(r) for r in rows.tolist()], s
            assert [[m[2] for m in e["matches"]] for e in h_log] == top_score.tolist(), s
            assert [[LC.STUDENT_IDS.index(m[0]) for m in e["matches"]] for e in h_log] == top_idx.tolist(), s
            assert h_info == [int(ids.max()) + 1 if len(ids) else 0, int((h_attempt >= 0).sum()), len(offsets) - 1, 0], s
            assert len(h_events) == sum(1 for e in log if e[4]["recognized"] or e[2] + 1 >= sess["max_attempts"]), s
            # and the mirror classes give the same files
            mine = ours.LiveFaceRecognition(similarity_threshold=sess["similarity_threshold"],
                                            output_dir=os.path.join(tmp, "live_mirror"), session_name=f"live_{s}",
                                            recognition_interval=sess["recognition_interval"],
                                            max_recognition_attempts=sess["max_attempts"],
                                            frame_buffer_size=sess["buffer_size"], processor=LC.ReplayProcessor(d),
                                            embedder=LC.PlanEmbedder(d), gallery=host_gallery, verbose=False)
            mine.max_distance = sess["max_distance"]
            mine.trace = trace
            m_ids, m_log = LC.drive(mine, d)
            assert np.array_equal(m_ids, ids) and [e[:4] for e in m_log] == [e[:4] for e in log], s
            with open(os.path.join(mine.session_dir, "attendance.json")) as f:
                assert LC.strip(json.load(f)) == attendance, s
            m_stats = mine._finalize_session()["statistics"]
            m_stats.pop("average_fps")
            assert m_stats == statistics, (s, m_stats, statistics)
            reached |= trace
            for name, v in (("track_id", ids), ("log", rows), ("log_top_idx", top_idx), ("log_top_score", top_score),
                            ("attendance", np.array(json.dumps(attendance))),
                            ("statistics", np.array(json.dumps(statistics))),
                            ("max_distance", np.float64(sess["max_distance"])),
                            ("recognition_interval", np.int32(sess["recognition_interval"])),
                            ("max_attempts", np.int32(sess["max_attempts"])),
                            ("buffer_size", np.int32(sess["buffer_size"])),
                            ("similarity_threshold", np.float64(sess["similarity_threshold"]))):
                d[name] = v
            for name, v in d.items():
                out[f"s{s}_{name}"] = v
            print("live session", s, "frames", len(offsets) - 1, "detections", len(ids), "tracks", h_info[0],
                  "attempts", len(log), "recognized", len(attendance["recognized"]), "unrecognized",
                  len(attendance["unrecognized"]), sorted(trace))
        assert reached >= LC.REQUIRED, sorted(LC.REQUIRED - reached)
        np.savez_compressed(os.path.join(OUT, "live_tracks.npz"), **out)
        print("live", len(built), "sessions;", os.path.getsize(os.path.join(OUT, "live_tracks.npz")), "bytes")

    if "evaluate" in parts:
        sys.path.insert(0, os.path.join(REPO, "tests"))
        import _eval_cases as EC
        from facerecognitionpipeline_amd import evaluate_models as EM
        wanted = ("cosine_similarity", "compute_all_similarities", "aggregate_max", "aggregate_mean", "aggregate_topk",
                  "identify_probe", "compute_rank_metrics", "compute_dprime", "bootstrap_confidence_interval",
                  "evaluate_probes_comprehensive", "evaluate_verification_comprehensive",
                  "evaluate_impostors_comprehensive", "evaluate_segmented_comprehensive")
        ns = {}
        exec("import numpy as np\nimport pandas as pd\nfrom typing import Dict, List, Tuple, Optional\n"
             "from sklearn.metrics import roc_curve, auc\ndef tqdm(it, **kw):\n    return it\n", ns)
        with open(os.path.join(REF, "evaluate_models_v2.ipynb")) as f:
            nb = json.load(f)
        for cell in nb["cells"]:  # the cells that define the functions, and nothing else of the notebook
            src = "".join(cell["source"])
            if cell["cell_type"] == "code" and any(f"def {n}(" in src for n in wanted):
                exec(compile(src, "evaluate_models_v2.ipynb", "exec"), ns)
        assert all(n in ns for n in wanted)
        f32 = np.float32

        def table(df, cols):
            assert list(df.columns) == list(cols), list(df.columns)
            return df[list(cols)].to_numpy(np.float64)

        def ver_arrays(ver, pre, out):
            out[pre + "ver_table"] = table(ver["threshold_results"], EC.VER_COLUMNS)
            out[pre + "ver_equal"] = np.array([ver[k] for k in EC.VER_EQUAL], np.float64)
            out[pre + "ver_float"] = np.array([ver[k] for k in EC.VER_FLOAT], np.float64)
            out[pre + "ver_genuine"] = np.array(ver["genuine_scores"], f32)
            out[pre + "ver_impostor"] = np.array(ver["impostor_scores"], f32)
            out[pre + "ver_auc_full"] = np.float64(EM.roc_curve_auc(ver["genuine_scores"], ver["impostor_scores"])[2])
            assert out[pre + "ver_auc_full"] == ver["roc_auc"], (pre, out[pre + "ver_auc_full"], ver["roc_auc"])

        out = {"labels": np.array([c["label"] for c in EC.all_cases()])}
        buckets = set()
        for case in EC.all_cases():
            label, gallery = case["label"], case["gallery"]
            gnames = list(gallery)
            thr = EC.thresholds_of(case)
            names, Q = EC.pack(case["positive"]["all"])
            nnames, NQ = EC.pack(case["negative"])
            _gn, E = EC.pack(gallery)
            offsets = EC.offsets_of(gallery)
            tid = EC.true_ids(names, gallery)
            exact = label.startswith("exact")
            out[f"{label}__sha256"] = np.array(EC.case_sha(case))
            out[f"{label}__thresholds"] = thr
            sim = np.array([[s for _n, s in ns["compute_all_similarities"](q, gallery)] for q in Q], f32)
            nsim = np.array([[s for _n, s in ns["compute_all_similarities"](q, gallery)] for q in NQ], f32)
            out[f"{label}__sim"], out[f"{label}__neg_sim"] = sim, nsim
            h_sim = EM.similarity_matrix_host(Q, E)
            if exact:
                assert h_sim.tobytes() == sim.tobytes(), label
            else:
                assert np.abs(h_sim - sim).max() <= EC.SCORE_TOL, (label, np.abs(h_sim - sim).max())
            for agg, k in case["runs"]:
                pre = f"{label}__{agg}{k}__"
                with quiet():
                    res = ns["evaluate_probes_comprehensive"](gallery, case["positive"], list(thr), aggregation=agg, k=k)
                    ver = ns["evaluate_verification_comprehensive"](gallery, case["positive"], case["negative"],
                                                                    list(thr), aggregation=agg, k=k)
                    imp = ns["evaluate_impostors_comprehensive"](gallery, case["negative"], list(thr),
                                                                 aggregation=agg, k=k)
                    nscores = np.array([[ns["identify_probe"](q, gallery, 0.0, agg, k)[2][g] for g in gnames]
                                        for q in NQ], f32)
                preds = res["all_predictions"]
                assert [p["true_identity"] for p in preds] == names
                scores = np.array([[p["identity_scores"][g] for g in gnames] for p in preds], f32)
                for p in preds:
                    assert all(type(v) is np.float32 for v in p["identity_scores"].values())
                rec_i = np.zeros((len(preds), 4), np.int32)
                rec_f = np.zeros((len(preds), 4), f32)
                for r, p in enumerate(preds):
                    ranked = sorted(p["identity_scores"].items(), key=lambda kv: kv[1], reverse=True)
                    rr = p["rank_metrics"]["reciprocal_rank"]
                    rank = int(round(1.0 / rr)) if rr > 0 else 0
                    assert (rank > 0) == (p["true_identity"] in gallery)
                    assert [p["rank_metrics"][f"rank{c}"] for c in (1, 5, 10)] == [1 <= rank <= c for c in (1, 5, 10)]
                    assert p["score"] == ranked[0][1]
                    others = [v for g, v in p["identity_scores"].items() if g != p["true_identity"]]
                    rec_i[r] = (gnames.index(p["predicted_identity"]) if p["predicted_identity"] is not None else -1,
                                gnames.index(ranked[0][0]), rank, 1 if others else 0)
                    rec_f[r] = (p["score"], p["identity_scores"].get(p["true_identity"], 0),
                                max(others) if others else -1.0, 0.0)
                    buckets.add((label.split("_")[0], 0 if rank == 0 else 1 if rank == 1 else 5 if rank <= 5 else
                                 10 if rank <= 10 else 11))
                tab = table(res["threshold_results"], EC.PROBE_COLUMNS)
                vtab = table(ver["threshold_results"], EC.VER_COLUMNS)
                counts = np.stack([tab[:, 11], tab[:, 12], tab[:, 13], vtab[:, 4]], axis=1).astype(np.int64)
                assert np.array_equal(counts, np.stack([tab[:, 11], tab[:, 12], tab[:, 13], vtab[:, 4]], axis=1))
                # the host statements are the reference, or the fixture is not written
                h_i, h_f, h_c = EM.eval_probes_host(scores, tid, thr)
                assert np.array_equal(h_i, rec_i) and h_f.tobytes() == rec_f.tobytes() and np.array_equal(h_c, counts), pre
                n_i, n_f, n_c = EM.eval_probes_host(nscores, np.full(len(nscores), -1, np.int32), thr)
                assert n_f[:, 0].tobytes() == np.array(imp["impostor_scores"], f32).tobytes(), pre
                assert np.array_equal(n_c[:, 2], table(imp["threshold_results"], EC.IMP_COLUMNS)[:, 3]), pre
                assert np.array_equal(n_c[:, 2], vtab[:, 6]), pre
                h_scores = EM.identity_scores_host(h_sim, offsets, agg, k)
                if exact:
                    assert h_scores.tobytes() == scores.tobytes(), pre
                else:
                    assert np.abs(h_scores - scores).max() <= EC.SCORE_TOL, (pre, np.abs(h_scores - scores).max())
                    EC.check_margins(scores, tid, nscores, thr, EC.float64_scores(Q, E, offsets, agg, k),
                                     EC.float64_scores(NQ, E, offsets, agg, k))
                out[pre + "scores"], out[pre + "neg_scores"] = scores, nscores
                out[pre + "rec_i"], out[pre + "rec_f"], out[pre + "counts"] = rec_i, rec_f, counts
                out[pre + "probe_table"] = tab
                pid = res["per_identity"]
                out[pre + "pid_names"] = np.array(list(pid))
                out[pre + "pid_table"] = np.array([[v["rank1"], v["rank5"], v["rank10"], v["mrr"], v["n_samples"]]
                                                   for v in pid.values()], np.float64)
                out[pre + "pid_genuine"] = np.array([s for v in pid.values() for s in v["genuine_scores"]], f32)
                out[pre + "pid_impostor_sum"] = np.array([np.sum(np.array(v["impostor_scores"], np.float64))
                                                          for v in pid.values()], np.float64)
                ver_arrays(ver, pre, out)
                out[pre + "imp_table"] = table(imp["threshold_results"], EC.IMP_COLUMNS)
                out[pre + "imp_stats"] = np.array([imp["mean_impostor_score"], imp["std_impostor_score"]], np.float64)
                out[pre + "dprime_fn"] = np.float64(ns["compute_dprime"](ver["genuine_scores"], ver["impostor_scores"]))
                segments = [s for s in case["positive"] if s != "all"]
                if segments:
                    with quiet():
                        seg = ns["evaluate_segmented_comprehensive"](gallery, case["positive"], case["negative"],
                                                                     list(thr), aggregation=agg, k=k)
                    assert list(seg) == segments
                    for sname, sres in seg.items():
                        out[pre + f"seg_{sname}__probe_table"] = table(sres["identification"]["threshold_results"],
                                                                       EC.PROBE_COLUMNS)
                        out[pre + f"seg_{sname}__predicted"] = np.array(
                            [gnames.index(p["predicted_identity"]) if p["predicted_identity"] is not None else -1
                             for p in sres["identification"]["all_predictions"]], np.int32)
                        ver_arrays(sres["verification"], pre + f"seg_{sname}__", out)
                print("evaluate", pre, "probes", len(preds), "rank1", tab[0, 1], "auc", ver["roc_auc"], "eer", ver["eer"])
            for k in case.get("topk_only", ()):
                with quiet():
                    sc = np.array([[ns["identify_probe"](q, gallery, 0.0, "topk", k)[2][g] for g in gnames] for q in Q], f32)
                assert np.abs(EM.identity_scores_host(h_sim, offsets, "topk", k) - sc).max() <= EC.SCORE_TOL
                out[f"{label}__topk{k}__scores_only"] = sc
        assert {b for lab, b in buckets if lab == "seeded"} == {0, 1, 5, 10, 11}, sorted(buckets)
        # bootstrap_confidence_interval: the reference draws from numpy's global generator; with the same
        # generator state the mirror draws the same samples
        data = [float(x) for x in np.linspace(0.1, 0.9, 23)]
        np.random.seed(1234)
        ci_ref = ns["bootstrap_confidence_interval"](data, n_bootstrap=200)
        np.random.seed(1234)
        assert EM.bootstrap_confidence_interval(data, n_bootstrap=200) == ci_ref
        out["bootstrap_data"], out["bootstrap_ci_seed1234_n200"] = np.array(data), np.array(ci_ref, np.float64)
        np.savez_compressed(os.path.join(OUT, "evaluate.npz"), **out)
        print("evaluate", len(out), "arrays;", os.path.getsize(os.path.join(OUT, "evaluate.npz")), "bytes")

    if "dropin" in parts:
        import shutil
        from facerecognitionpipeline_amd.gallery_manager import GalleryManager as DropIn
        d = os.path.join(tmp, "dropin")
        os.makedirs(d)
        shutil.copyfile(os.path.join(OUT, "ref_students.pkl"), os.path.join(d, "students.pkl"))
        ours = DropIn(gallery_path=os.path.join(d, "students.pkl"), verbose=False)
        sids = list(ours.students)
        r = np.random.Generator(np.random.PCG64(0xFACE0D1D))

        def unit(n):
            x = r.standard_normal((n, 512)).astype(np.float32)
            return x / np.linalg.norm(x, axis=1, keepdims=True)

        ours.add_student("NEW0001", "Enrolled Through The Drop-In", unit(3), metadata={"source": "frhip"})
        ours.update_embeddings(sids[1], unit(2), mode="append")
        ours.delete_student(sids[2])
        ours.save()
        shutil.copyfile(os.path.join(d, "students.pkl"), os.path.join(OUT, "dropin_students.pkl"))
        with quiet():
            ref = ref_gm.GalleryManager(gallery_path=os.path.join(d, "students.pkl"))  # the reference's load
        ids = list(ref.students)
        recs = [{"student_id": x.student_id, "name": x.name, "num_samples": int(x.num_samples),
                 "enrollment_date": x.enrollment_date, "last_updated": x.last_updated, "metadata": x.metadata,
                 "class": type(x).__module__ + "." + type(x).__name__,
                 "embeddings_sha256": sha(np.asarray(x.embeddings)), "embeddings_dtype": str(x.embeddings.dtype),
                 "template_sha256": sha(np.asarray(x.template_embedding))} for x in ref.students.values()]
        queries = np.concatenate([np.asarray(x.embeddings, np.float32) for x in ref.students.values()])
        gal, idx, sc = search_arrays(ref, queries)
        np.savez_compressed(os.path.join(OUT, "dropin_students.npz"), ids=np.array(ids),
                            records=np.array(json.dumps(recs)), queries_sha256=np.array(sha(queries)),
                            search_idx=idx, search_score=sc, gallery_sha256=np.array(sha(gal.astype(np.float32))))
        print("dropin", len(ids), "students read back by the reference; queries", queries.shape)


if __name__ == "__main__":
    main()
