"""vba_options::lm_trial_launches without a GPU: the field fills the four bytes of alignment padding between the execution knobs'
five ints and max_map_nodes, so no other field's offset and not the struct's size depend on it, and a zeroed struct means the default."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_field_fills_the_padding_and_defaults_to_zero():
    import voxel_slam_amd  # noqa: F401
    from voxel_slam_amd import capi
    O = capi.Options
    assert O.lm_trial_launches.offset == O.hessian_compact_tiles.offset + C.sizeof(C.c_int)
    assert O.max_map_nodes.offset == O.lm_trial_launches.offset + C.sizeof(C.c_int)
    assert O.max_map_nodes.offset % C.sizeof(C.c_size_t) == 0          # (so the slot was padding before the field existed)
    without = type("Without", (C.Structure,), {"_fields_": [f for f in O._fields_ if f[0] != "lm_trial_launches"]})
    assert C.sizeof(without) == C.sizeof(O)
    for name, _ in without._fields_:
        assert getattr(without, name).offset == getattr(O, name).offset, name
    assert capi.default_options().lm_trial_launches == 0


def test_header_declares_the_field_where_the_binding_has_it():
    hdr = open(os.path.join(ROOT, "include", "voxelba.h")).read()
    body = re.search(r"typedef struct vba_options \{(.*?)\} vba_options;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"\b([a-z_0-9]+)(?:\[\d+\])?;", body)
    from voxel_slam_amd import capi
    assert fields == [f[0] for f in capi.Options._fields_]
