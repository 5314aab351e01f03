"""Host-side checks of the criterion-list entry points (no GPU needed): argument errors come back as codes with a message, and
loss.fuse_criterion_list picks the pair path, the criterion-list path or none."""
import ctypes as C

import pytest
import torch


@pytest.fixture(scope="module")
def lib():
    import os
    from brats2019_amd import _lib as L
    if not os.path.exists(L.LIB_PATH):
        from brats2019_amd import build
        build.build(verbose=False)
    return L.load()


def test_crit_entry_points_reject_bad_arguments(lib):
    from brats2019_amd import _lib as L
    dummy = C.c_void_p(16)                       # never dereferenced: every call below fails its argument check first
    assert lib.ru_crit_moments_workspace_bytes(0, 3, 100) == 0
    cases = [
        ("ru_crit_moments", lambda: lib.ru_crit_moments(None, dummy, 1, 3, 100, L.CRIT_MASK_ALL, dummy, dummy, 1 << 20, None)),
        ("ru_crit_moments", lambda: lib.ru_crit_moments(dummy, dummy, 1, 3, 0, L.CRIT_MASK_ALL, dummy, dummy, 1 << 20, None)),
        ("ru_crit_moments", lambda: lib.ru_crit_moments(dummy, dummy, 1, 3, 100, 0x80, dummy, dummy, 1 << 20, None)),
        ("ru_crit_moments", lambda: lib.ru_crit_moments(dummy, dummy, 1, 3, 100, L.CRIT_MASK_ALL, dummy, dummy, 0, None)),
        ("ru_crit_reduce", lambda: lib.ru_crit_reduce(None, 1, 3, dummy, None)),
        ("ru_crit_reduce", lambda: lib.ru_crit_reduce(dummy, 0, 3, dummy, None)),
        ("ru_crit_eval", lambda: lib.ru_crit_eval(dummy, dummy, 1, 3, 10.0, 1.0, C.cast((L.CritTerm * 1)(L.CritTerm(1, 1.0, 1.0, 1.0)), C.c_void_p),
                                                  0, dummy, dummy, None)),
        ("ru_crit_eval", lambda: lib.ru_crit_eval(dummy, dummy, 1, 3, 10.0, 1.0, C.cast((L.CritTerm * 1)(L.CritTerm(99, 1.0, 1.0, 1.0)), C.c_void_p),
                                                  1, dummy, dummy, None)),
        ("ru_crit_eval", lambda: lib.ru_crit_eval(dummy, dummy, 2, 3, 10.0, 1.0, C.cast((L.CritTerm * 1)(L.CritTerm(1, 1.0, 1.0, 1.0)), C.c_void_p),
                                                  1, dummy, dummy, None)),
        ("ru_crit_grad", lambda: lib.ru_crit_grad(dummy, None, dummy, None, 1, 3, 100, 1, dummy, None)),
        ("ru_crit_grad", lambda: lib.ru_crit_grad(dummy, dummy, dummy, None, 70000, 3, 100, 1, dummy, None)),
    ]
    for name, call in cases:
        rc = call()
        assert rc < 0, name
        msg = L.last_error()
        assert name in msg, (name, msg)


def test_fuse_criterion_list_paths():
    from brats2019_amd import loss as L
    pair = L.fuse_criterion_list([L.BCE_Loss(bg_weight=1e-2), L.Dice_loss_joint()])
    assert pair is not None and pair.__qualname__ == "fuse_criterion_list.<locals>.run"        # the existing one-pass pair path
    terms = L.fuse_criterion_list([L.GDL_joint(), L.BCE_Loss(bg_weight=1e-2)])
    assert terms is not None and terms.__qualname__ == "_fuse_terms.<locals>.run"
    assert L.fuse_criterion_list((L.Dice_loss_separate(), L.Dice1D(), L.sens_loss_joint(), L.CE_Loss(), L.MSE_Loss())) is not None
    assert L.fuse_criterion_list([L.GDL_joint(), torch.nn.MSELoss()]) is None                     # a foreign module
    assert L.fuse_criterion_list([L.GDL_joint(index=0), L.MSE_Loss(index=1)]) is None             # two tensor indices
    assert L.fuse_criterion_list([L.Dice_loss_joint()]) is None                                   # alone it hands over to the network
    assert L.fuse_criterion_list([L.GDL_joint()] * 9) is None                                     # more terms than one launch takes
    assert L.fuse_criterion_list(L.GDL_joint()) is None
    dp = L.GDL_joint()
    dp.data_parallel = True
    assert L.fuse_criterion_list([dp, L.MSE_Loss()]) is None


def test_new_criteria_keep_the_reference_surface():
    from brats2019_amd import loss as L
    m = L.MSE_Loss()
    assert (m.index, m.priority, m.data_parallel) == (0, 1, False)
    assert L.CE_Loss(index=2).index == 2
    assert L.Dice1D().label_index == 0
    for cls in (L.GDL_joint, L.sens_loss_joint, L.Dice_loss_separate):
        c = cls(index=1, priority=3)
        assert (c.index, c.priority) == (1, 3) and isinstance(c, L._LossBase)
    with pytest.raises(AssertionError):
        L.GDL_joint()([torch.zeros(1, 3, 2, 2, 2)], [torch.zeros(1, 3, 2, 2, 3)])
