"""The loaded FK of retraction robots is reachable from every layer's public names: the C ABI list (tests/test_host.py holds it against
the header and the library's exports), the engine's methods."""
NEW_ABI = ("tr_fk_loaded_batch_retraction_dev", "tr_set_loaded_retraction")


def test_new_calls_are_exported(irt):
    assert set(NEW_ABI) <= set(irt._lib.ABI_SYMBOLS)
    header = open(irt._lib.HEADER).read()
    for name in NEW_ABI:
        assert "int %s(" % name in header, name
    for name in ("set_loaded_retraction", "fk_loaded_batch_retraction_dev", "validate_shapes_retraction_dev", "validate_loaded"):
        assert callable(getattr(irt.Engine, name)), name
