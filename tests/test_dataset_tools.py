"""The probe dataset tools (host code): ``ProbeSegmenter`` and ``DatasetPreprocessor`` against what
the reference modules gave on the same inputs (tests/golden/segment_dataset.npz and
dataset_preprocessor.npz, written by tools/make_golden_dataset.py from the inputs of
tests/_dataset_cases.py), and both command lines.  No GPU: the preprocessor runs with a stub processor.
"""
import json
import os

import numpy as np
import pytest

from tests import _dataset_cases as DC

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")


@pytest.fixture(scope="module")
def seg_golden():
    return np.load(os.path.join(GOLDEN, "segment_dataset.npz"))


def _segmenter(**kw):
    from facerecognitionpipeline_amd.segment_dataset import ProbeSegmenter
    return ProbeSegmenter(verbose=False, **kw)


def test_exports():
    import facerecognitionpipeline_amd as pkg
    from facerecognitionpipeline_amd.dataset_preprocessor import DatasetPreprocessor
    from facerecognitionpipeline_amd.segment_dataset import ProbeSegmenter
    assert pkg.DatasetPreprocessor is DatasetPreprocessor and pkg.ProbeSegmenter is ProbeSegmenter
    assert {"DatasetPreprocessor", "ProbeSegmenter"} <= set(pkg.__all__)


@pytest.mark.parametrize("setting", list(DC.SEGMENTER_SETTINGS))
@pytest.mark.parametrize("tag", ["full", "one"])
def test_segmenter_thresholds_and_categories(seg_golden, setting, tag):
    full = DC.metadata_list()
    assert DC.sha_json(full) == str(seg_golden["metadata_sha256"]) and len(full) == int(seg_golden["n"])
    lst = full if tag == "full" else full[41:42]
    seg = _segmenter(**DC.SEGMENTER_SETTINGS[setting])
    seg.compute_blur_thresholds(lst)
    want = seg_golden[f"{setting}__{tag}__thresholds"]
    got = np.array([seg.blur_sharp_threshold, seg.blur_blurry_threshold], np.float64)
    assert got.tobytes() == want.tobytes(), (got, want)
    if setting == "idx_at_len":
        assert seg.blur_sharp_threshold == 0 and seg.blur_blurry_threshold == 0
    cats = json.loads(str(seg_golden[f"{setting}__{tag}__categories"]))
    assert len(cats) == len(lst)
    for m, c in zip(lst, cats):
        assert seg.categorize_face(m) == c, m["filename"]
    if setting == "default" and tag == "full":
        assert {x for c in cats for x in c} == set(seg.categories)  # every bucket is exercised


def test_segmenter_quirks():
    seg = _segmenter(det_score_threshold=0.5)
    seg.blur_sharp_threshold = seg.blur_blurry_threshold = 100.0
    m = {"yaw": 0.0, "pitch": 0.0, "blur_score": 100.0, "det_score": 0.6, "face_size": 200}
    cats = seg.categorize_face(m)
    assert "blur_sharp" in cats and "blur_blurry" in cats            # both tests are inclusive
    assert "baseline" not in cats and "low_quality" not in cats       # baseline uses the literal 0.7
    assert "baseline" in seg.categorize_face(dict(m, det_score=0.7))


@pytest.mark.parametrize("copy_files", [True, False])
def test_segment_dataset_run(seg_golden, tmp_path, copy_files):
    picked, files = DC.segment_run_list()
    assert DC.sha_json([picked, sorted(files)]) == str(seg_golden["run_sha256"])
    src, meta = DC.write_segment_inputs(str(tmp_path / "in"), picked, files)
    dst = str(tmp_path / "segmented")
    seg = _segmenter()
    seg.segment_dataset(input_dir=src, metadata_file=meta, output_dir=dst, copy_files=copy_files)
    run = json.loads(str(seg_golden["run"]))
    assert sorted(os.listdir(dst)) == sorted(seg.categories) == sorted(run)
    n_files = 0
    for c in seg.categories:
        with open(os.path.join(dst, c, f"{c}_metadata.json")) as f:
            text = f.read()
        assert text == run[c]["metadata"], c
        names = sorted(n for n in os.listdir(os.path.join(dst, c)) if n != f"{c}_metadata.json")
        assert names == run[c]["files"], c
        for n in names:
            p = os.path.join(dst, c, n)
            assert os.path.islink(p) == (not copy_files)
            with open(p, "rb") as f, open(os.path.join(src, n), "rb") as g:
                assert f.read() == g.read()
        n_files += len(names)
    assert n_files > len(picked)
    rows = [r for c in run.values() for r in json.loads(c["metadata"])]
    assert any(r.get("labeled_filename", "").startswith("labeled_S017_") for r in rows)   # endswith match
    assert any("labeled_filename" not in r for r in rows)                                  # entry with no file
    seg.segment_dataset(input_dir=src, metadata_file=meta, output_dir=dst, copy_files=copy_files)  # again: replaces


def test_segmenter_main_and_parser(tmp_path, capsys):
    from facerecognitionpipeline_amd import segment_dataset as SD
    a = SD.build_parser().parse_args([])
    assert (a.input_dir, a.metadata_file, a.output_dir) == (
        "output/preprocessed/probe_positive", "output/preprocessed/probe_positive_metadata.json",
        "output/preprocessed/segmented")
    assert (a.pose_easy_threshold, a.pose_medium_threshold, a.face_large_threshold, a.face_medium_threshold,
            a.blur_sharp_percentile, a.blur_blurry_percentile, a.det_score_threshold, a.symlink) == (
        15.0, 30.0, 150, 80, 50.0, 20.0, 0.7, False)
    assert (a.yaw_threshold, a.pitch_threshold, a.blur_threshold) == (35.0, 25.0, 50.0)
    picked, files = DC.segment_run_list()
    src, meta = DC.write_segment_inputs(str(tmp_path / "in"), picked, files)
    SD.main(["--input_dir", src, "--metadata_file", meta, "--output_dir", str(tmp_path / "out"), "--symlink",
             "--face_large_threshold", "120", "--det_score_threshold", "0.5"])
    want = SD.ProbeSegmenter(face_large_threshold=120, det_score_threshold=0.5, verbose=False)
    want.compute_blur_thresholds(picked)
    with open(tmp_path / "out" / "face_large" / "face_large_metadata.json") as f:
        large = [m["filename"] for m in json.load(f)]
    assert large == [m["filename"] for m in picked if "face_large" in want.categorize_face(m)]
    assert any(119 < m.get("face_size", 0) < 150 for m in picked if m["filename"] in large)  # the flag took effect
    assert os.path.islink(tmp_path / "out" / "face_large" / large[0])
    assert "Quality Insights" in capsys.readouterr().out
    assert os.path.exists(tmp_path / "out" / "baseline" / "baseline_metadata.json")


# ---------------------------------------------------------------------------- DatasetPreprocessor
class BatchStub:
    """A processor with FaceProcessor.process_images' contract and fixed answers."""

    def __init__(self):
        self.calls = []

    def process_images(self, images, return_all=False, errors="raise"):
        assert return_all is True and errors == "return"
        self.calls.append(len(images))
        return [DC.faces_for(np.asarray(im)) for im in images]


class PerImageStub:
    """The reference's contract only: process_image(path, return_all)."""

    def process_image(self, image_path, return_all=False):
        from facerecognitionpipeline_amd.face_recognition import load_image_rgb
        img = load_image_rgb(image_path)
        if img is None:
            raise ValueError(f"Could not load image: {image_path}")
        return DC.faces_for(img)


@pytest.fixture(scope="module")
def pre_golden():
    g = np.load(os.path.join(GOLDEN, "dataset_preprocessor.npz"))
    assert DC.sha_json(DC.TREE) == str(g["tree_sha256"])
    return g


@pytest.mark.parametrize("stub,batch_size", [(BatchStub, 4), (BatchStub, 1), (BatchStub, 64), (PerImageStub, 3)])
def test_preprocessor_matches_reference(pre_golden, tmp_path, stub, batch_size):
    from PIL import Image
    from facerecognitionpipeline_amd.dataset_preprocessor import DatasetPreprocessor
    tree = DC.build_tree(str(tmp_path / "classroom"))
    proc = stub()
    pre = DatasetPreprocessor(processor=proc, batch_size=batch_size, verbose=False)
    out = str(tmp_path / "out")
    assert pre.process_dataset(input_dir=tree, output_dir=out) is None
    with open(os.path.join(out, "probe_positive_metadata.json")) as f:
        text = f.read()
    assert text == str(pre_golden["metadata"])                       # keys, key order, types, entry order
    names = sorted(os.listdir(os.path.join(out, "probe_positive")))
    assert names == json.loads(str(pre_golden["files"]))
    for n in names:
        with Image.open(os.path.join(out, "probe_positive", n)) as im:
            assert im.size == (224, 224) and im.format == "JPEG"
    meta = json.loads(text)
    n_images = sum(1 for rel, _red in DC.TREE if rel.count("/") >= 1 and not rel.startswith("top_level")
                   and os.path.splitext(rel)[1].lower() in (".png", ".bmp", ".jpg", ".jpeg"))
    assert len(meta) == len(names) == 12
    if stub is BatchStub:  # bounded chunks; the undecodable file is never handed on
        assert max(proc.calls) <= batch_size and sum(proc.calls) == n_images - 1


def test_preprocessor_batch_failure_loses_one_image_only(tmp_path):
    from facerecognitionpipeline_amd.dataset_preprocessor import DatasetPreprocessor

    class Fragile(BatchStub):
        def process_images(self, images, return_all=False, errors="raise"):
            if any(im.shape[0] == 31 for im in images):  # one size is refused whatever call holds it
                raise ValueError("image too small to letterbox")
            return super().process_images(images, return_all, errors)

    tree = DC.build_tree(str(tmp_path / "classroom"))
    out = str(tmp_path / "out")
    DatasetPreprocessor(processor=Fragile(), batch_size=5, verbose=False).process_dataset(tree, out)
    with open(os.path.join(out, "probe_positive_metadata.json")) as f:
        got = json.load(f)
    want = json.loads(str(np.load(os.path.join(GOLDEN, "dataset_preprocessor.npz"))["metadata"]))
    from facerecognitionpipeline_amd.face_recognition import load_image_rgb
    lost = {os.path.basename(rel) for rel, red in DC.TREE
            if red is not None and load_image_rgb(os.path.join(tree, rel)).shape[0] == 31}
    assert lost and got == [m for m in want if m["source_image"] not in lost]


def test_preprocessor_raises_what_is_no_argument_error(tmp_path):
    """A device error (RuntimeError) or a processor without ``errors=`` (TypeError) must not be retried
    image by image or counted as 0 faces: it ends the walk."""
    from facerecognitionpipeline_amd.dataset_preprocessor import DatasetPreprocessor

    class Faulted(BatchStub):
        def process_images(self, images, return_all=False, errors="raise"):
            self.calls.append(len(images))
            raise RuntimeError("HIP error: an illegal memory access was encountered")

    class OldSignature:
        def process_images(self, images, return_all=False):
            return [[] for _ in images]

    tree = DC.build_tree(str(tmp_path / "classroom"))
    proc = Faulted()
    with pytest.raises(RuntimeError):
        DatasetPreprocessor(processor=proc, batch_size=5, verbose=False).process_dataset(tree, str(tmp_path / "o1"))
    assert len(proc.calls) == 1
    with pytest.raises(TypeError):
        DatasetPreprocessor(processor=OldSignature(), verbose=False).process_dataset(tree, str(tmp_path / "o2"))


def test_preprocessor_single_image_and_names(tmp_path):
    from facerecognitionpipeline_amd.dataset_preprocessor import DatasetPreprocessor
    tree = DC.build_tree(str(tmp_path / "classroom"))
    pre = DatasetPreprocessor(processor=BatchStub(), verbose=False)
    assert pre.standardize_filename("x/y.png", "class_a", "left", 7) == "class_a_left_007.jpg"
    meta = []
    os.makedirs(tmp_path / "o")
    n = pre.process_single_image(os.path.join(tree, "class_a/center/b_second.png"), "class_a", "center",
                                 "class_a_center_002", str(tmp_path / "o"), meta)
    assert n == 1 and [m["filename"] for m in meta] == ["class_a_center_002_face0.jpg"]
    assert pre.process_single_image(os.path.join(tree, "class_b/broken.jpeg"), "class_b", "center", "b", str(tmp_path / "o"),
                                    meta) == 0 and len(meta) == 1
    assert pre.process_dataset(str(tmp_path / "o"), str(tmp_path / "o2")) is None   # no class directories
    with pytest.raises(ValueError):
        DatasetPreprocessor(processor=BatchStub(), batch_size=0)


def test_preprocessor_main_and_parser(tmp_path):
    from facerecognitionpipeline_amd import dataset_preprocessor as DP
    a = DP.build_parser().parse_args([])
    assert (a.input_dir, a.output_dir, a.probe_dir, a.metadata_file, a.output_size, a.det_thresh, a.batch_size) == (
        "samples/classroom", "output/preprocessed", "probe_positive", "probe_positive_metadata.json", 224, 0.3, 32)
    tree = DC.build_tree(str(tmp_path / "classroom"))
    out = str(tmp_path / "out")
    assert a.detector_model is None
    DP.main(["--input_dir", tree, "--output_dir", out, "--probe_dir", "p", "--metadata_file", "m.json",
             "--batch_size", "2"], processor=BatchStub())
    with open(os.path.join(out, "m.json")) as f:
        assert len(json.load(f)) == 12
    assert len(os.listdir(os.path.join(out, "p"))) == 12
