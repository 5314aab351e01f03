"""The resident training set without a GPU: the box and kind rules (`pack_case_host`, the numpy restatement of `ru_case_probe`), the argument checks
of `ResidentCases` and `augment_batch` that fire before any device call, and the new names in the header and in the ctypes table."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPE = (2, 5, 6, 7)


def blank():
    return np.zeros(SHAPE, np.float32), np.zeros(SHAPE[1:], np.uint8)


def test_box_touches_a_volume_face():
    from brats2019_amd import dataloader as DL
    image, label = blank()
    image[0, 0, 2, 3] = 7.0                                   # on the D = 0 face
    image[1, 3, 5, 6] = 9.0                                   # on the far H and W faces
    assert DL.pack_case_host(image, label) == ((0, 2, 3), (4, 4, 4), "uint16")


def test_label_and_soft_outside_the_image_box_widen_it():
    from brats2019_amd import dataloader as DL
    image, label = blank()
    image[0, 2:4, 2:4, 2:4] = 3.0
    assert DL.pack_case_host(image, label) == ((2, 2, 2), (2, 2, 2), "uint16")
    label[1, 3, 5] = 2                                        # a label voxel outside the image's box
    assert DL.pack_case_host(image, label) == ((1, 2, 2), (3, 2, 4), "uint16")
    soft = np.zeros((3,) + SHAPE[1:], np.float32)
    assert DL.pack_case_host(image, label, soft) == ((1, 2, 2), (3, 2, 4), "uint16")
    soft[2, 4, 0, 6] = 1e-30                                  # a non-zero soft value outside both
    assert DL.pack_case_host(image, label, soft) == ((1, 0, 2), (4, 4, 5), "uint16")
    soft[2, 4, 0, 6] = 0.0
    soft[0, 2, 2, 0] = -0.0                                   # by bit pattern: -0.0 counts
    assert DL.pack_case_host(image, label, soft) == ((1, 2, 0), (3, 2, 6), "uint16")


def test_all_zero_case():
    from brats2019_amd import dataloader as DL
    image, label = blank()
    assert DL.pack_case_host(image, label) == ((0, 0, 0), (1, 1, 1), "uint16")
    assert DL.pack_case_host(image, label, np.zeros((3,) + SHAPE[1:], np.float32)) == ((0, 0, 0), (1, 1, 1), "uint16")


@pytest.mark.parametrize("value,kind", [(0.5, "float32"), (-1.0, "float32"), (65536.0, "float32"), (-0.0, "float32"), (float("nan"), "float32"),
                                        (0.0, "uint16"), (65535.0, "uint16")])
def test_kind_rule(value, kind):
    from brats2019_amd import dataloader as DL
    image, label = blank()
    image[0, 1:3, 1:3, 1:3] = 100.0
    image[1, 2, 2, 2] = value
    lo, size, got = DL.pack_case_host(image, label)
    assert got == kind
    assert (lo, size) == ((1, 1, 1), (2, 2, 2))               # the trigger sits inside the box the other channel spans


def test_the_trigger_alone_is_inside_the_box():
    """-0.0 and NaN are not +0.0 by bit pattern: each spans a box of its own"""
    from brats2019_amd import dataloader as DL
    for value in (-0.0, float("nan")):
        image, label = blank()
        image[1, 4, 5, 6] = value
        assert DL.pack_case_host(image, label) == ((4, 5, 6), (1, 1, 1), "float32")


def test_pack_case_host_refuses_bad_shapes():
    from brats2019_amd import dataloader as DL
    image, label = blank()
    with pytest.raises(ValueError):
        DL.pack_case_host(image[0], label)
    with pytest.raises(ValueError):
        DL.pack_case_host(image, label[1:])
    with pytest.raises(ValueError):
        DL.pack_case_host(image, label, np.zeros((2,) + SHAPE[1:], np.float32))


def test_resident_cases_argument_checks_come_before_the_device():
    from brats2019_amd import dataloader as DL
    called = []
    cases = [lambda: called.append(1)]
    with pytest.raises(ValueError, match="dtype"):
        DL.ResidentCases(cases, (8, 8, 8), dtype="float16")
    for bad in (-1, 1.5, "1G", True):
        with pytest.raises(ValueError, match="max_bytes"):
            DL.ResidentCases(cases, (8, 8, 8), max_bytes=bad)
    with pytest.raises(ValueError, match="patch_size"):
        DL.ResidentCases(cases, (8, 8))
    assert not called                                         # no case was read
    empty = DL.ResidentCases([], (8, 8, 8), max_bytes=0)      # an empty store needs no device
    assert len(empty) == 0 and empty.nbytes == 0 and empty.patch_size == (8, 8, 8)


class _Store(object):
    """what `augment_batch` reads of a store before its first device call"""

    def __init__(self, n, patch):
        self.n, self.patch_size = n, patch

    def __len__(self):
        return self.n

    def __getitem__(self, i):
        raise AssertionError("augment_batch touched a case before its argument checks passed")


def _params(transpose=False, **extra):
    p = dict(crop_lo=np.array([1, 2, 3]), scale=np.ones(3), flips=[False, True, False], transpose=transpose, gain=np.ones(4), bias=np.zeros(4))
    p.update(extra)
    return p


def test_augment_batch_argument_checks_come_before_the_device():
    from brats2019_amd import dataloader as DL
    with pytest.raises(ValueError, match="transposed"):
        DL.augment_batch(_Store(3, (8, 9, 8)), [0, 1], [_params(), _params(transpose=True)])
    with pytest.raises(ValueError, match="elastic"):
        DL.augment_batch(_Store(3, (8, 8, 8)), [0, 1], [_params(elastic=dict(sigma=12.0, alpha=300.0, seed=1)), _params()])
    with pytest.raises(ValueError, match="index"):
        DL.augment_batch(_Store(3, (8, 8, 8)), [0, 3], [_params(), _params()])
    with pytest.raises(ValueError, match="one parameter dict per index"):
        DL.augment_batch(_Store(3, (8, 8, 8)), [0, 1], [_params()])
    with pytest.raises(ValueError, match="at least one sample"):
        DL.augment_batch(_Store(3, (8, 8, 8)), [], [])
    with pytest.raises(ValueError, match="singular"):         # the affine checks of the single-patch path
        DL.augment_batch(_Store(3, (8, 8, 8)), [0], [_params(rotation=dict(matrix=np.zeros((3, 3))))])


def test_resident_loader_refuses_a_list_reader():
    from brats2019_amd import dataloader as DL
    image, label = blank()
    with pytest.raises(ValueError, match="ResidentCases"):
        DL.ResidentLoader(DL.SimpleReader([(image, label)], (2, 2, 2)), batch_size=2)
    with pytest.raises(ValueError, match="built for patch"):
        DL.SimpleReader(DL.ResidentCases([], (8, 8, 8)), (4, 4, 4))


def test_new_names_in_header_and_ctypes_table():
    from brats2019_amd import _lib as L
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "resunet_hip.h")).read(), flags=re.S)
    for name in ("ru_case_probe", "ru_case_pack", "ru_case_unpack", "ru_augment_batch_packed"):
        assert re.search(r"\b%s\s*\(" % name, src), name
        assert name in L.SIGNATURES, name
    defines = dict(re.findall(r"#define\s+(RU_\w+)\s+(-?\d+)", src))
    assert (int(defines["RU_PACK_F32"]), int(defines["RU_PACK_U16"])) == (L.PACK_F32, L.PACK_U16)
    assert (int(defines["RU_AUG_ZOOM"]), int(defines["RU_AUG_AFFINE"])) == (L.AUG_ZOOM, L.AUG_AFFINE)
    assert int(defines["RU_AUG_BATCH_MAX"]) == L.AUG_BATCH_MAX >= 1
    # the descriptors as the C compiler lays them out (LP64): the launch's argument block holds RU_AUG_BATCH_MAX samples under HIP's 4 KB
    assert C.sizeof(L.CaseDesc) == 136 and C.sizeof(L.PatchDesc) == 208
    assert L.AUG_BATCH_MAX * (C.sizeof(L.CaseDesc) + C.sizeof(L.PatchDesc)) < 4096
