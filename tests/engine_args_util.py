"""A stand-in for an engine's library that proves an argument was refused before the C ABI: shared by the emulated and the GPU
argument tests."""
import contextlib


class LibGuard:
    """Forwards dqmc_last_error (Engine._check reads it); any other entry point raises AssertionError, so a check that lets a
    bad argument through fails the test instead of handing a wrong pointer to the library."""

    def __init__(self, lib):
        self._lib = lib

    def __getattr__(self, name):
        if name == 'dqmc_last_error':
            return self._lib.dqmc_last_error
        raise AssertionError(f'{name} was reached: the argument was not refused before the library')


@contextlib.contextmanager
def guarded(eng):
    real = eng.lib
    eng.lib = LibGuard(real)
    try:
        yield eng
    finally:
        eng.lib = real
