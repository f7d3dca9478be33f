"""CPU: the entry points of include/omnipq_data.h are exported by both libraries with typed signatures, and every refusal the
header lists comes back before the device is touched: the pointers below are never dereferenced, and this machine has no GPU
to launch on."""
import ctypes

import capi
from test_capi_symbols import both

EINVAL, ETOOLARGE = 10001, 10002
P = 0x1000                               # "some non-null pointer"


def structs():
    import device_data as D
    bank = D._Bank(4, 4, 3, 1000, P, P, P, P, P, P, P, P)
    batch = D._Batch(2, 1024, 0, 18, 18, P, P, P, None, None, P, P)
    out = D._Out(*[P] * len(D.OUT_FIELDS))
    return D, bank, batch, out


def call(lib, bank, batch, out, workspace=P):
    def ref(s):
        return ctypes.c_void_p(ctypes.addressof(s)) if s is not None else ctypes.c_void_p(0)
    return lib.omnipq_assemble_batch(ref(bank), ref(batch), ref(out), ctypes.c_void_p(workspace), ctypes.c_void_p(0))


def test_symbols_are_exported_and_typed(built_lib):
    want = capi.declared_signatures()
    assert want["omnipq_assemble_batch"] == ("i", "ppppp")
    assert want["omnipq_assemble_workspace_bytes"] == ("l", "i")
    for path in both(built_lib):
        lib = ctypes.CDLL(path)
        got = capi.reported_signatures(lib)
        for name in ("omnipq_assemble_batch", "omnipq_assemble_workspace_bytes"):
            assert hasattr(lib, name) and got[name] == want[name], (path, name)
        assert lib.omnipq_abi_version() == 5                 # additive: the version stays
    import pointnet2_utils
    ext = pointnet2_utils._load_ext()
    assert ext._lib.omnipq_assemble_batch.restype is ctypes.c_int
    assert list(ext._lib.omnipq_assemble_batch.argtypes) == [ctypes.c_void_p] * 5


def test_struct_layouts_match_the_header(built_lib):
    """the module's three descriptors have the header's fields in the header's order (include/omnipq_data.h as
    capi.declared_records reads it: test_capi_symbols guards the whole report), and OUT_FIELDS names exactly the arrays of
    omnipq_asm_out"""
    D, *_ = structs()
    declared = capi.declared_records()[1]
    kinds = {ctypes.c_void_p: "p", ctypes.c_longlong: "l", ctypes.c_int: "i"}
    for cls, name in ((D._Bank, "omnipq_asm_bank"), (D._Batch, "omnipq_asm_batch"), (D._Out, "omnipq_asm_out")):
        assert [(n, kinds[t], None) for n, t in cls._fields_] == declared[name], name
    assert len(D._Out._fields_) == 31
    assert sorted(f[0] for f in D.OUT_FIELDS) == sorted(n for n, _ in D._Out._fields_) and len(D.OUT_FIELDS) == 31
    assert (D.META_INTS, D.LABEL_DOUBLES, D.PARAM_DOUBLES) == (8, 64 * 7 + 32 * 8 + 48, 12)


def test_workspace_bytes(built_lib):
    lib = capi.lib()
    lib.omnipq_assemble_workspace_bytes.restype = ctypes.c_longlong
    per_item = 1024 * 8 * 4 + 1024 * 4 * 4 + 64 * 3 * 8
    assert lib.omnipq_assemble_workspace_bytes(1) == per_item and lib.omnipq_assemble_workspace_bytes(16) == 16 * per_item
    assert lib.omnipq_assemble_workspace_bytes(0) == 0 and lib.omnipq_assemble_workspace_bytes(-3) == 0
    assert lib.omnipq_assemble_workspace_bytes(65536) == 0


def test_every_refusal_comes_before_the_device(built_lib):
    lib = capi.lib()
    D, bank, batch, out = structs()

    def with_(struct, **kw):
        c = type(struct).from_buffer_copy(struct)
        for k, v in kw.items():
            setattr(c, k, v)
        return c

    assert call(lib, None, batch, out) == EINVAL and call(lib, bank, None, out) == EINVAL
    assert call(lib, bank, batch, None) == EINVAL
    for kw in ({"b": -1}, {"k": 0}, {"flavour": 2}, {"flavour": -1}, {"n_ids": -1}, {"n_sizes": 0}, {"scene_slot": None},
               {"params": None}, {"seed": None}, {"mean_size": None}, {"nyu40ids": None}):
        assert call(lib, bank, with_(batch, **kw), out) == EINVAL, kw
    assert call(lib, bank, with_(batch, seed=None, choices_in=P), out) == EINVAL        # the teacher's draw still needs it
    for kw in ({"scenes": 0}, {"pitch": 2}, {"height_col": 2}, {"height_col": 4}, {"height_col": -2}, {"rows_total": -1},
               {"points": None}, {"normals": None}, {"instance": None}, {"semantic": None}, {"row_offset": None},
               {"meta": None}, {"labels": None}):
        assert call(lib, with_(bank, **kw), batch, out) == EINVAL, kw
    for key in ("point_clouds", "vertex_normals", "ema_point_clouds", "choices", "ema_choices", "semantic_labels", "vote_label",
                "vote_label_mask", "point_instance_label", "center_label", "size_class_label", "num_gt_boxes", "gt_quad_sizes",
                "horizontal_quads", "flip_x_axis", "rot_mat", "scale", "scan_idx"):
        assert call(lib, bank, batch, with_(out, **{key: None})) == EINVAL, key
    assert call(lib, bank, batch, out, workspace=0) == EINVAL
    unl = with_(batch, flavour=1, n_ids=0, n_sizes=0, nyu40ids=None, mean_size=None)
    assert call(lib, bank, unl, with_(out, size_label=None)) == EINVAL
    for kw in ({"b": 65536}, {"k": (1 << 24) + 1}, {"n_ids": 65}):
        assert call(lib, bank, with_(batch, **kw), out) == ETOOLARGE, kw
    assert call(lib, with_(bank, pitch=9, height_col=-1), batch, out) == ETOOLARGE
    # b == 0 succeeds and does nothing, whatever the pointers
    assert call(lib, bank, with_(batch, b=0), out) == 0
    assert call(lib, with_(bank, points=None), with_(batch, b=0, seed=None), with_(out, point_clouds=None), workspace=0) == 0
