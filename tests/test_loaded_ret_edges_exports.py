"""The second level of opening and the shooting's order report are reachable from every layer's public names: the C ABI list
(tests/test_host.py holds it against the header and the library's exports), the header's level constants, the engine's methods."""
import inspect

NEW_ABI = ("tr_loaded_retraction", "tr_loaded_order_last")


def test_new_calls_are_exported(irt):
    assert set(NEW_ABI) <= set(irt._lib.ABI_SYMBOLS)
    header = open(irt._lib.HEADER).read()
    for name in NEW_ABI:
        assert "int %s(" % name in header, name
    for name in ("TR_LOADED_RETRACTION_OFF = 0", "TR_LOADED_RETRACTION_FK = 1", "TR_LOADED_RETRACTION_EDGES = 2",
                 "TENDON_HIP_LOADED_RETRACT_SORT"):
        assert name in header, name
    for name in ("set_loaded_retraction", "loaded_retraction", "loaded_order_last"):
        assert callable(getattr(irt.Engine, name)), name
    sig = inspect.signature(irt.Engine.set_loaded_retraction)
    assert sig.parameters["on"].default is True and sig.parameters["edges"].default is False
