"""The text of the shape refusals of the five voxel-map entries (epcnet_map_fuse, epcnet_map_surfels, epcnet_surfel_map_init / _add /
_move): `<entry>: need ...` for num_rows, num_clouds and max_voxels out of range, in that order where more than one is.  The refusals are
host-side and come before any launch: the addresses are never followed, so no device is needed."""
import ctypes

import pytest

import helpers as H

A = 0x10000
ROWS, CLOUDS, VOXELS = "need 0 <= num_rows < 2^31", "need 0 <= num_clouds <= 2^24", "need 1 <= max_voxels <= 2^28"
CASES = [(dict(rows=-1), ROWS), (dict(rows=1 << 31), ROWS), (dict(clouds=-1), CLOUDS), (dict(clouds=(1 << 24) + 1), CLOUDS),
         (dict(voxels=0), VOXELS), (dict(voxels=(1 << 28) + 1), VOXELS),
         (dict(rows=-1, clouds=-1, voxels=0), ROWS), (dict(clouds=-1, voxels=0), CLOUDS)]


def _call(entry, rows=1000, clouds=4, voxels=1000):
    lib = H.pkg("lib").lib()
    map_params = (ctypes.c_double * 8)(0.2, 1.0, *([0.0] * 6))
    params = (ctypes.c_double * 8)(0.2, 1.0, 1.0, 8.0, *([0.0] * 4))
    if entry == "epcnet_map_fuse":
        return lib.epcnet_map_fuse(A, A, rows, clouds, A, A, map_params, voxels, A, A, A, A, 0, None)
    if entry == "epcnet_map_surfels":
        return lib.epcnet_map_surfels(A, A, rows, clouds, A, A, params, voxels, A, A, A, A, A, A, A, A, 0, None)
    if entry == "epcnet_surfel_map_init":
        return lib.epcnet_surfel_map_init(A, params, voxels, A, 0, A, A, A, A, A, A, A, None)
    if entry == "epcnet_surfel_map_add":
        return lib.epcnet_surfel_map_add(A, A, rows, clouds, A, params, voxels, A, 0, A, A, A, A, A, A, A, A, A, 0, None)
    return lib.epcnet_surfel_map_move(A, A, rows, clouds, A, A, params, voxels, A, 0, A, A, A, A, A, A, A, A, A, 0, None)


@pytest.mark.parametrize("entry", ["epcnet_map_fuse", "epcnet_map_surfels", "epcnet_surfel_map_init", "epcnet_surfel_map_add",
                                   "epcnet_surfel_map_move"])
def test_shape_refusals_word_for_word(entry):
    L = H.pkg("lib")
    cases = [c for c in CASES if set(c[0]) == {"voxels"}] if entry == "epcnet_surfel_map_init" else CASES      # init takes no rows
    for kw, message in cases:
        assert _call(entry, **kw) == L.EPC_EINVAL, kw
        assert L.lib().epc_last_error() == ("%s: %s" % (entry, message)).encode(), kw
    # the largest shape in range reaches the next refusal: a state, or a workspace, of 0 bytes
    assert _call(entry, rows=(1 << 31) - 1, clouds=1 << 24, voxels=1 << 28) == L.EPC_ENOMEM
