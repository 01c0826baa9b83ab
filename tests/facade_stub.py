"""A stand-in for the device context under ``SketchClient`` (shared by the CPU
tests of the facade; no fixture lives here, so it is a plain module)."""


class StubContext:
    """Stands where the device context would: records the native calls the
    facade makes and answers success, so what is checked is what the facade
    does on its own (dispatch, argument checks, key table, call sequence).

    ``calls`` holds the call names; ``log`` holds ``[name, arg, ...]`` with the
    int / float arguments as they are, None as None and anything else (arrays,
    structs, pointers) as ``"*"``.  Output arrays stay as the caller zeroed
    them unless ``hooks[name]``, called with the arguments, writes to them.  A
    name in ``fail`` raises ``SketchLibError(code, text)`` after it was
    recorded."""

    def __init__(self, lib, fail=None):
        self.lib, self.ptr, self.calls, self.log = lib, None, [], []
        self.fail = dict(fail or {})
        self.hooks = {}

    def call(self, name, *args):
        self.calls.append(name)
        self.log.append([name] + [_scalar(a) for a in args])
        if name in self.fail:
            from rtsas_amd import SketchLibError
            raise SketchLibError(*self.fail[name])
        if name in self.hooks:
            self.hooks[name](*args)
        return 0


def _scalar(a):
    if a is None or isinstance(a, (bool, float)):
        return a
    if isinstance(a, int):
        return int(a)
    if hasattr(a, "dtype") and getattr(a, "shape", None) == ():  # a numpy scalar
        return a.item()
    return "*"
