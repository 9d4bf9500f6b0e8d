"""CPU-only: the C-ABI library loads and exports its header; host-side logic of the mirrors."""
import os
import re

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared(header):
    with open(os.path.join(REPO, "include", header)) as f:
        src = f.read()
    return sorted(set(re.findall(r"^\s*(?:const\s+)?[a-z_0-9]+\s*\*?\s*((?:fr|frt)_[a-z_0-9]+)\s*\(", src, re.M)))


def test_library_loads_and_exports_every_declared_symbol():
    from facerecognitionpipeline_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        from facerecognitionpipeline_amd.build import build
        build(verbose=False)
    lib = _lib.load()
    names = _declared("frhip.h") + _declared("frhip_testing.h")
    assert len(names) >= 18, names
    for n in names:
        assert hasattr(lib, n), f"libfrhip.so does not export {n}"
    assert b"gfx950" in lib.fr_version()


def test_capi_reports_errors_without_gpu():
    import ctypes
    from facerecognitionpipeline_amd import _lib
    lib = _lib.load()
    h = ctypes.c_void_p()
    assert lib.fr_create(b"ir_7", b"adaface", 0, 8, ctypes.byref(h)) == _lib.FR_ERR_INVALID_ARGUMENT
    assert b"Unknown architecture" in lib.fr_last_error(None)
    assert lib.fr_create(b"ir_50", b"resnet", 0, 8, ctypes.byref(h)) == _lib.FR_ERR_INVALID_ARGUMENT
    assert b"Unknown model_type" in lib.fr_last_error(None)
    with pytest.raises(ValueError):
        _lib.check(_lib.FR_ERR_INVALID_ARGUMENT)


def test_product_refuses_cpu_device():
    import torch
    from facerecognitionpipeline_amd import _lib
    with pytest.raises(RuntimeError):
        _lib.Handle("ir_50", "adaface", torch.device("cpu"))


def _gm(tmp_path):
    from facerecognitionpipeline_amd.gallery_manager import GalleryManager
    return GalleryManager(gallery_path=str(tmp_path / "g" / "students.npz"), verbose=False)


def test_gallery_records_and_templates(tmp_path, golden_dir):
    from oracle.reference_path import aggregate_template
    f = np.load(os.path.join(golden_dir, "backup_adaface_ir_101.npz"))
    gm = _gm(tmp_path)
    for sid, e in zip(f["student_ids"][:5], f["embeddings"][:5]):
        assert gm.add_student(str(sid), str(sid), e)
    assert not gm.add_student(str(f["student_ids"][0]), "x", f["embeddings"][0])
    E, ids = gm.get_gallery_embeddings()
    assert ids == [str(s) for s in f["student_ids"][:5]]
    assert np.array_equal(E, f["ref_template"][:5])
    for method in ("median", "weighted_mean"):
        gm.aggregation_method = method
        t = gm._aggregate_embeddings(f["embeddings"][0])
        assert np.abs(t - aggregate_template(f["embeddings"][0], method)).max() <= 1e-7
    gm.aggregation_method = "mean"
    sid = str(f["student_ids"][1])
    assert gm.update_embeddings(sid, f["embeddings"][6][:2], mode="append")
    assert gm.get_student(sid).num_samples == 10
    assert gm.update_embeddings(sid, f["embeddings"][6], mode="replace")
    assert gm.get_student(sid).num_samples == 8
    assert gm.update_embeddings(sid, f["embeddings"][7], mode="merge")
    with pytest.raises(ValueError):
        gm.update_embeddings(sid, f["embeddings"][7], mode="bogus")
    assert gm.delete_student(sid) and not gm.delete_student(sid)
    st = gm.get_statistics()
    assert st["num_students"] == 4
    # save/load round trip (one npz with every field)
    gm.save()
    gm2 = _gm(tmp_path)
    assert list(gm2.students) == list(gm.students)
    for s in gm.students:
        assert np.array_equal(gm2.students[s].template_embedding, gm.students[s].template_embedding)
    out = gm.export_for_backup(str(tmp_path / "bk"), "t")
    gm3 = _gm(tmp_path / "x")
    gm3.load_backup(out)
    assert np.allclose(gm3.get_gallery_embeddings()[0], gm.get_gallery_embeddings()[0])


def test_build_templates_argument_errors_without_gpu():
    """fr_build_templates checks its arguments before the handle, like the other CSR batch calls, so
    a NULL handle still gets a text that names the bad argument."""
    import ctypes
    from facerecognitionpipeline_amd import _lib
    lib = _lib.load()
    emb = (ctypes.c_float * (8 * 512))()
    tpl = (ctypes.c_float * (2 * 512))()
    kept = (ctypes.c_int32 * 2)()
    max_samples = 1024  # frhip.h: 1..1024 rows per student

    def call(emb=emb, offsets=(0, 3, 8), n_students=2, method=0, tpl=tpl):
        off = (ctypes.c_int32 * len(offsets))(*offsets) if offsets is not None else None
        rc = lib.fr_build_templates(None, emb, off, n_students, method, 0.7, tpl, kept, None)
        return rc, lib.fr_last_error(None)

    for kw, text in (({}, b"NULL handle"), ({"n_students": 0, "offsets": None}, b"NULL handle"),
                     ({"emb": None}, b"NULL buffer"), ({"offsets": None}, b"NULL buffer"),
                     ({"tpl": None}, b"NULL buffer"), ({"n_students": -1}, b"n_students"),
                     ({"method": 3}, b"method"), ({"method": -1}, b"method"),
                     ({"offsets": (1, 3), "n_students": 1}, b"offsets[0]"),
                     ({"offsets": (0, 0, 2)}, b"student 0 has 0"),           # empty student
                     ({"offsets": (0, 3, 2)}, b"student 1 has -1"),          # decreasing offsets
                     ({"offsets": (0, max_samples + 1), "n_students": 1}, b"student 0 has 1025"),
                     ({"offsets": (0, 1, -2**31)}, b"student 1 has -2147483649")):   # lengths do not wrap
        rc, msg = call(**kw)
        assert rc == _lib.FR_ERR_INVALID_ARGUMENT, kw
        assert text in msg, (kw, msg)
    assert not any(tpl) and not any(kept)  # nothing was written


def test_reference_backup_json_loads(tmp_path, golden_dir):
    """A reference export_for_backup JSON reproduces the fixture templates."""
    import json
    f = np.load(os.path.join(golden_dir, "backup_arcface_ir_50.npz"))
    data = {"students": {str(s): {"student_id": str(s), "name": str(s), "embeddings": e.tolist(),
                                  "template_embedding": t.tolist(), "num_samples": 8, "enrollment_date": "",
                                  "last_updated": "", "metadata": {}}
                         for s, e, t in zip(f["student_ids"], f["embeddings"], f["stored_template"])}}
    p = tmp_path / "b.json"
    p.write_text(json.dumps(data))
    gm = _gm(tmp_path)
    gm.load_backup(str(p))
    E, _ = gm.get_gallery_embeddings()
    assert np.array_equal(E.astype(np.float32), f["stored_template"])


def test_reference_gallery_pickle_loads(tmp_path, golden_dir):
    """The reference's own gallery file (pickle.dump(self.students), gallery_manager.py:207-210),
    written by the reference GalleryManager (tools/make_golden.py refpkl), loads through the
    restricted unpickler: every record field, templates equal to the reference's own."""
    import json
    import shutil
    from facerecognitionpipeline_amd.gallery_manager import GalleryManager
    f = np.load(os.path.join(golden_dir, "backup_adaface_ir_101.npz"))
    d = tmp_path / "gallery"
    d.mkdir()
    shutil.copyfile(os.path.join(golden_dir, "ref_students.pkl"), d / "students.pkl")
    shutil.copyfile(os.path.join(golden_dir, "ref_students.json"), d / "students.json")
    ref_json = (d / "students.json").read_text()
    gm = GalleryManager(gallery_path=str(d / "students.pkl"), verbose=False)
    E, ids = gm.get_gallery_embeddings()
    assert ids == [str(s) for s in f["student_ids"]]
    assert np.array_equal(E, f["ref_template"])
    meta = json.loads(ref_json)["students"]
    for sid, r in gm.students.items():
        assert r.name == meta[sid]["name"] and r.num_samples == meta[sid]["num_samples"] == 8
        assert r.enrollment_date == meta[sid]["enrollment_date"] and r.metadata == meta[sid]["metadata"]
        assert r.embeddings.shape == (8, 512)
    # a save of the unchanged gallery rewrites the reference's file byte for byte
    # (gallery_manager.py:207-210 pickle.dump of the same records) ...
    pkl_bytes = (d / "students.pkl").read_bytes()
    gm.save()
    assert (d / "students.pkl").read_bytes() == pkl_bytes
    # ... and after a deletion, the reference-format .pkl, this module's .npz and the sidecar
    # all hold the new gallery
    assert gm.delete_student(ids[0])
    gm.save()
    from facerecognitionpipeline_amd.gallery_manager import load_reference_pickle
    assert list(load_reference_pickle(str(d / "students.pkl"))) == ids[1:]
    side = json.loads((d / "students.json").read_text())
    assert set(side) == set(json.loads(ref_json)) and list(side["students"]) == ids[1:]
    assert set(side["students"][ids[1]]) == set(meta[ids[1]])
    gm2 = GalleryManager(gallery_path=str(d / "students.pkl"), verbose=False)
    assert list(gm2.students) == ids[1:]
    assert np.array_equal(gm2.get_gallery_embeddings()[0], f["ref_template"][1:])
    assert not [p for p in os.listdir(d) if p.endswith(".tmp")]


def test_dropin_pickle_is_what_the_reference_reads(tmp_path, golden_dir):
    """tests/golden/dropin_students.pkl was written by THIS module's save (the reference's file
    loaded, a student enrolled / updated / deleted through the drop-in) and read back by the
    REFERENCE GalleryManager (tools/make_golden.py dropin): the records it saw and its search of
    every stored sample are in dropin_students.npz.  Here: the same records load through the
    restricted unpickler, re-saving writes the same bytes, and the reference's search results are
    the oracle search of these templates (the GPU search is checked in test_gpu_gallery.py)."""
    import hashlib
    import json
    import shutil
    from facerecognitionpipeline_amd.gallery_manager import GalleryManager
    from oracle import reference_path as rp
    fx = np.load(os.path.join(golden_dir, "dropin_students.npz"))
    recs = json.loads(str(fx["records"]))
    shutil.copyfile(os.path.join(golden_dir, "dropin_students.pkl"), tmp_path / "students.pkl")
    gm = GalleryManager(gallery_path=str(tmp_path / "students.pkl"), verbose=False)
    sha = lambda a: hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()  # noqa: E731
    assert list(gm.students) == [str(x) for x in fx["ids"]] and "NEW0001" in gm.students
    for want, r in zip(recs, gm.students.values()):
        assert want["class"] == "gallery_manager.StudentRecord"
        assert (r.student_id, r.name, r.num_samples, r.enrollment_date, r.last_updated, r.metadata) == (
            want["student_id"], want["name"], want["num_samples"], want["enrollment_date"], want["last_updated"],
            want["metadata"])
        assert sha(r.embeddings) == want["embeddings_sha256"] and str(r.embeddings.dtype) == want["embeddings_dtype"]
        assert sha(r.template_embedding) == want["template_sha256"]
    gm.save()
    assert (tmp_path / "students.pkl").read_bytes() == open(os.path.join(golden_dir, "dropin_students.pkl"), "rb").read()
    E, ids = gm.get_gallery_embeddings()
    assert sha(E.astype(np.float32)) == str(fx["gallery_sha256"])
    q = np.concatenate([np.asarray(r.embeddings, np.float32) for r in gm.students.values()])
    assert sha(q) == str(fx["queries_sha256"])
    names = {s: gm.students[s].name for s in ids}
    for i in range(0, len(q), 7):
        res = rp.search(E, ids, names, q[i], top_k=5)
        assert [ids.index(s) for s, _n, _sc in res] == fx["search_idx"][i].tolist()
        assert np.abs(np.array([sc for _s, _n, sc in res]) - fx["search_score"][i]).max() <= 1e-6


def test_gallery_file_choice_follows_the_recorded_pickle_signature(tmp_path, golden_dir, caplog):
    """when both <stem>.npz and <stem>.pkl exist, load takes the .npz unless the .pkl
    differs from the one saved with it -- file times do not decide (a copy or checkout resets
    them) -- and says which it took."""
    import logging
    import shutil
    import time
    from facerecognitionpipeline_amd.gallery_manager import GalleryManager
    p = tmp_path / "students.pkl"
    rng = np.random.default_rng(5)
    gm = GalleryManager(gallery_path=str(p), verbose=False)
    for i in range(4):
        gm.add_student(f"S{i}", f"N{i}", rng.standard_normal((2, 512)).astype(np.float32))
    gm.save()
    assert p.exists() and (tmp_path / "students.npz").exists()
    t = time.time() + 100
    os.utime(p, (t, t))  # the .pkl looks newer, but it is the one saved with the .npz
    caplog.set_level(logging.WARNING)
    assert GalleryManager._source(str(p))[0] == "npz"
    assert "loading the .npz" in caplog.text
    # save without the reference file: an existing .pkl stays as it is, the .npz is preferred
    gm.add_student("S9", "N9", rng.standard_normal((1, 512)).astype(np.float32))
    old_pkl = p.read_bytes()
    gm.save(reference_pickle=False)
    assert p.read_bytes() == old_pkl
    assert list(GalleryManager(gallery_path=str(p), verbose=False).students) == ["S0", "S1", "S2", "S3", "S9"]
    # the reference app rewrites the .pkl: that is the newer gallery, whatever the file times say
    shutil.copyfile(os.path.join(golden_dir, "ref_students.pkl"), p)
    os.utime(p, (1, 1))
    assert GalleryManager._source(str(p))[0] == "pkl"
    assert "STU0001" in GalleryManager(gallery_path=str(p), verbose=False).students


def test_export_for_backup_copies_the_gallery_files(tmp_path, golden_dir):
    """gallery_manager.py:246-270: the backup holds a copy of the gallery file (the reference's
    .pkl; this module's .npz too when there is one) and the JSON export; with no gallery file
    it raises FileNotFoundError before writing anything."""
    import json
    import shutil
    from facerecognitionpipeline_amd.gallery_manager import GalleryManager
    d = tmp_path / "g"
    d.mkdir()
    shutil.copyfile(os.path.join(golden_dir, "ref_students.pkl"), d / "students.pkl")
    gm = GalleryManager(gallery_path=str(d / "students.pkl"), verbose=False)
    out = gm.export_for_backup(str(tmp_path / "b1"), "adaface")
    got = sorted(os.listdir(tmp_path / "b1"))
    assert len(got) == 2 and got[1].endswith(".pkl") and got[0].endswith(".json") and got[1].startswith("adaface_backup_")
    assert (tmp_path / "b1" / got[1]).read_bytes() == (d / "students.pkl").read_bytes()
    assert json.load(open(out))["num_students"] == len(gm.students)
    gm.save()
    gm.export_for_backup(str(tmp_path / "b2"))
    assert sorted(os.path.splitext(x)[1] for x in os.listdir(tmp_path / "b2")) == [".json", ".npz", ".pkl"]
    empty = GalleryManager(gallery_path=str(tmp_path / "none" / "students.pkl"), verbose=False)
    empty.add_student("S0", "N0", np.ones((1, 512), np.float32))
    with pytest.raises(FileNotFoundError):
        empty.export_for_backup(str(tmp_path / "b3"))
    assert not os.listdir(tmp_path / "b3")


def test_saved_gallery_files_keep_the_usual_mode(tmp_path):
    """the atomic writes keep the mode of the file they replace, and a new file gets
    0666 & ~umask (as open() would), not mkstemp's 0600."""
    import stat
    from facerecognitionpipeline_amd.gallery_manager import GalleryManager, _UMASK
    p = tmp_path / "students.pkl"
    gm = GalleryManager(gallery_path=str(p), verbose=False)
    gm.add_student("S0", "N0", np.ones((1, 512), np.float32))
    gm.save()
    for f in ("students.pkl", "students.npz", "students.json"):
        assert stat.S_IMODE(os.stat(tmp_path / f).st_mode) == 0o666 & ~_UMASK, f
    os.chmod(tmp_path / "students.npz", 0o640)
    gm.save()
    assert stat.S_IMODE(os.stat(tmp_path / "students.npz").st_mode) == 0o640


def test_gallery_pickle_with_foreign_globals_raises(tmp_path):
    """A pickle naming anything outside numpy's array reconstruction and the reference's
    StudentRecord raises before it is resolved; an unreadable gallery never loads as empty."""
    import pickle
    from facerecognitionpipeline_amd.gallery_manager import GalleryManager
    d = tmp_path / "g"
    d.mkdir()
    bad = [b"cos\nsystem\n(S'echo pwned > /dev/null'\ntR.",           # protocol 0 GLOBAL os.system
           b"\x80\x04cbuiltins\neval\n(S'1+1'\ntR.",                 # builtins.eval
           pickle.dumps({"S1": 3}),                                  # not a StudentRecord
           pickle.dumps([1, 2]),                                     # not a dict
           b"not a pickle at all"]
    for i, blob in enumerate(bad):
        (d / "students.pkl").write_bytes(blob)
        with pytest.raises((pickle.UnpicklingError, ValueError, EOFError)):
            GalleryManager(gallery_path=str(d / "students.pkl"), verbose=False)


def test_save_uses_unique_temporaries_and_one_file(tmp_path):
    """Two managers saving the same path concurrently each land a complete, loadable file."""
    import threading
    from facerecognitionpipeline_amd.gallery_manager import GalleryManager
    p = str(tmp_path / "s" / "students.npz")
    rng = np.random.default_rng(3)
    mgrs = []
    for m in range(2):
        gm = GalleryManager(gallery_path=str(tmp_path / f"src{m}" / "x.npz"), verbose=False)
        for i in range(6 + m):
            gm.add_student(f"S{m}{i}", f"N{i}", rng.standard_normal((2, 512)).astype(np.float32))
        mgrs.append(gm)
    ts = [threading.Thread(target=lambda g=g: [g.save(p) for _ in range(5)]) for g in mgrs]
    [t.start() for t in ts]
    [t.join() for t in ts]
    out = GalleryManager(gallery_path=p, verbose=False)
    assert list(out.students) in ([f"S0{i}" for i in range(6)], [f"S1{i}" for i in range(7)])
    assert not [q for q in os.listdir(tmp_path / "s") if q.endswith(".tmp")]


def test_slice_semantics_of_top_k():
    from facerecognitionpipeline_amd.gallery_manager import _slice_len
    assert [_slice_len(3, k) for k in (5, 3, 1, 0, -1, -5)] == [3, 3, 1, 0, 2, 0]


def test_torch_library_ops_shapes_without_gpu():
    """frhip::embed / match_topk / embed_match are registered torch ops whose
    fake implementations give the output shapes (traceable without running a kernel)."""
    import torch
    from torch._subclasses.fake_tensor import FakeTensorMode
    from facerecognitionpipeline_amd import torch_ops  # noqa: F401  (registers the ops)
    with FakeTensorMode():
        x = torch.empty(6, 112, 112, 3, dtype=torch.uint8)
        e = torch.ops.frhip.embed(x, 1, True)
        assert e.shape == (6, 512) and e.dtype == torch.float32
        i, s = torch.ops.frhip.match_topk(e, 1, 5)
        assert i.shape == (6, 5) and i.dtype == torch.int32 and s.dtype == torch.float32
        i, s, e2 = torch.ops.frhip.embed_match(x, 1, 3)
        assert i.shape == (6, 3) and e2.shape == (6, 512)
    with pytest.raises(ValueError):
        torch.ops.frhip.embed(torch.zeros(1, 112, 112, 3, dtype=torch.uint8), 10 ** 6, True)


def test_gallery_delta_replays_random_mutations(tmp_path):
    """pending_delta + apply_gallery_delta_matrix reproduce get_gallery_embeddings after any
    sequence of add / overwrite / update / delete (the incremental HBM sync's contract)."""
    import torch
    from facerecognitionpipeline_amd.gallery_manager import GalleryManager, apply_gallery_delta_matrix

    class TagOnly:
        device = torch.device("cpu")
        gallery_tag = None

    rng = np.random.default_rng(11)
    gm = GalleryManager(gallery_path=str(tmp_path / "g" / "s.npz"), verbose=False)
    gm.attach_handle(TagOnly())
    for i in range(4):
        gm.add_student(f"S{i}", "n", rng.normal(size=(2, 512)).astype(np.float32))
    assert gm.pending_delta() is None          # nothing on the device yet: full upload
    E = torch.from_numpy(gm.get_gallery_embeddings()[0].astype(np.float32))
    gm._mark_synced(list(gm.students))
    nxt = 4
    for _round in range(30):
        for _ in range(int(rng.integers(1, 6))):
            op = rng.integers(0, 4)
            ids = list(gm.students)
            if op == 0 or not ids:
                gm.add_student(f"S{nxt}", "n", rng.normal(size=(int(rng.integers(1, 5)), 512)).astype(np.float32))
                nxt += 1
            elif op == 1:
                gm.add_student(ids[rng.integers(len(ids))], "m", rng.normal(size=(3, 512)).astype(np.float32),
                               overwrite=True)
            elif op == 2:
                gm.update_embeddings(ids[rng.integers(len(ids))], rng.normal(size=(1, 512)).astype(np.float32))
            else:
                gm.delete_student(ids[rng.integers(len(ids))])
        d = gm.pending_delta()
        assert d is not None
        ops, rows, new_ids = d
        E = apply_gallery_delta_matrix(E, ops, rows)
        want = gm.get_gallery_embeddings()[0]
        assert new_ids == list(gm.students)
        assert np.array_equal(E.numpy(), np.asarray(want, np.float32).reshape(-1, 512))
        gm._mark_synced(new_ids)
    gm._touch()  # a bulk change (load / load_backup) always falls back to a full upload
    assert gm.pending_delta() is None


def test_match_batcher_routes_concurrent_requests():
    """MatchBatcher (pipeline.py) on a stand-in matcher: every concurrent caller gets its own
    result, cut to its own top_k with slice semantics; requests are batched; a wrong-shape
    crop raises ValueError in the caller; a failing batch fails each of its callers."""
    import threading
    import types

    from facerecognitionpipeline_amd.pipeline import MatchBatcher

    class FakeMatcher:
        def __init__(self):
            self.gallery = types.SimpleNamespace(students={f"S{i}": None for i in range(6)})
            self.embedder = types.SimpleNamespace(_check_shape=self._check)
            self.fail = False
            self.gate = threading.Event()

        @staticmethod
        def _check(f):
            if f.shape != (112, 112, 3):
                raise ValueError("bad shape")

        def match_faces(self, faces, top_k=5):
            self.gate.wait(5)
            if self.fail:
                raise RuntimeError("device failure")
            # "match" = the crop's tag pixel, repeated top_k times with descending scores
            return [[(f"S{int(f[0, 0, 0])}", "n", 1.0 - j / 10) for j in range(top_k)] for f in faces]

    fm = FakeMatcher()
    with MatchBatcher(fm, max_batch=8, max_wait_ms=20) as mb:
        crops = [np.full((112, 112, 3), i % 6, np.uint8) for i in range(24)]
        ks = [1 + i % 4 for i in range(23)] + [-2]  # -2: slice semantics -> 4 of 6 rows
        futs = [mb.submit(c, k) for c, k in zip(crops, ks)]
        fm.gate.set()
        for i, (f, k) in enumerate(zip(futs, ks)):
            r = f.result(timeout=10)
            assert len(r) == len(range(6)[:k])
            assert all(x[0] == f"S{i % 6}" for x in r)
        assert sum(mb.batches) == 24 and max(mb.batches) <= 8 and len(mb.batches) < 24
        with pytest.raises(ValueError):
            mb.submit(np.zeros((50, 50, 3), np.uint8))
        fm.fail = True
        with pytest.raises(RuntimeError, match="device failure"):
            mb.match_single_face(crops[0], 3)
    with pytest.raises(RuntimeError, match="closed"):
        mb.submit(crops[0])


def test_non_uint8_crops_only_at_input_size():
    """Float / 16-bit crops convert exactly only at 112x112; at other sizes the reference resizes them
    in their own dtype (cv2.resize, face_embedder.py:94-96), so the uint8 device path refuses them."""
    from facerecognitionpipeline_amd.face_embedder import as_uint8_crop
    rng = np.random.default_rng(0)
    ok = rng.integers(0, 256, (112, 112, 3)).astype(np.float64)
    assert np.array_equal(as_uint8_crop(ok), ok.astype(np.uint8))
    assert as_uint8_crop(ok.astype(np.uint16)).dtype == np.uint8
    for bad in (rng.integers(0, 256, (224, 200, 3)).astype(np.float64),
                rng.integers(0, 256, (224, 224, 3)).astype(np.uint16)):
        with pytest.raises(ValueError, match="must already be 112x112"):
            as_uint8_crop(bad)
    with pytest.raises(ValueError):
        as_uint8_crop(ok + 0.5)
    u8 = rng.integers(0, 256, (224, 200, 3), dtype=np.uint8)
    assert as_uint8_crop(u8) is u8  # uint8 of any size goes to the device resize unchanged


def test_bench_c4_frames_are_seeded():
    """bench.py's C4 frames and landmark placements are a function of the seed (the JSON line
    says "seeded"): two calls agree, another seed differs."""
    import torch

    import bench
    dev = torch.device("cpu")
    f1, l1 = bench.c4_inputs(9, 8, dev)
    f2, l2 = bench.c4_inputs(9, 8, dev)
    f3, _ = bench.c4_inputs(9, 8, dev, seed=8)
    assert f1.shape == (2, 1080, 1920, 3) and f1.dtype == torch.uint8
    assert torch.equal(f1, f2) and all(np.array_equal(a, b) for a, b in zip(l1, l2))
    assert not torch.equal(f1, f3)
