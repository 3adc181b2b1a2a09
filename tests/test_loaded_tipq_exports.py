"""The tip queries on loaded shapes are reachable from every layer's public names: the C ABI list (tests/test_host.py holds it against
the header and the library's exports), the package's export list, the classes' methods."""
NEW_ABI = ("tr_roadmap_ik_batch_loaded", "tr_roadmap_solve_tips_loaded", "tr_roadmap_set_tips_loaded", "tr_fk_loaded_tips", "tr_fk_loaded_tips_dev")


def test_new_calls_are_exported(irt):
    assert set(NEW_ABI) <= set(irt._lib.ABI_SYMBOLS)
    header = open(irt._lib.HEADER).read()
    for name in NEW_ABI:
        assert "int %s(" % name in header, name
    assert "chained_plan_loaded" in irt.__all__ and callable(irt.chained_plan_loaded)
    for name in ("roadmap_ik_loaded_batch", "solve_to_tips_loaded", "set_tips_loaded"):
        assert callable(getattr(irt.VoxelCachedLazyPRM, name)), name
    for name in ("fk_loaded_tips", "fk_loaded_tips_dev"):
        assert callable(getattr(irt.Engine, name)), name
    assert callable(irt.tip_control.loaded_tips_batch_device)
