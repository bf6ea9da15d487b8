"""Check the device mixins against the reference aggregator classes, as recorded from the REAL reference in
tests/golden/reference_aggregator_signatures.json: for every method the checks below look at, its parameter list
(names, kinds, defaults) and the class that defines it (``__qualname__``).  The classes are rebuilt from that record
as stand-ins of the same names, MRO and method signatures, so the checks run wherever the repository is.

    python tests/golden/check_mixin_vs_reference.py            # against the record
    python tests/golden/check_mixin_vs_reference.py --live     # against the reference checkout itself
    python tests/golden/check_mixin_vs_reference.py --record   # rewrite the record from the reference checkout

(--live and --record need the reference checkout gen_golden.py names, with the off-path placeholders it installs.)
Run by tests/test_mixin_vs_reference.py in a child process.
For ``class A(DeviceAggregatorMixin, Aggregator)`` (fedscale/cloud/aggregation/aggregator.py) it checks that
* every method the mixin overrides exists on the reference class with the same parameter list (names,
  kinds, defaults), so the reference event loop's calls bind to the mixin unchanged;
* ``_reference_impl(name)`` is True for each of them: the next method in the MRO is the reference's own, so
  the mixin takes its device path (and a plugin that overrides one keeps its own);
* ``super()`` from the mixin reaches ``Aggregator.init_model`` (aggregator.py:198-211) and the MRO places
  the mixin first;
* tests/event_loop.py's restatement of the reference loop has the same parameter lists as the reference for
  every method it restates, and its class name makes ``_reference_impl`` behave as with the real class.
For ``class B(DeviceAsyncAggregatorMixin, AsyncAggregator)`` (async_aggregator.py) it checks that FedBuff's own
``create_client_task`` (:40) is recognised as a plugin override (``_reference_impl`` False), and the same
parameter-list checks; for Auxo (examples/auxo/aggregator.py:451-472) the cohort mixin's signatures.
Prints one JSON report; exit status 1 on any mismatch.
"""
from __future__ import annotations

import inspect
import json
import os
import sys

os.environ["PYTHONDONTWRITEBYTECODE"] = "1"
sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)

RECORD = os.path.join(HERE, "reference_aggregator_signatures.json")

#: methods the aggregator mixin overrides (fedscale_amd/cloud/aggregation/aggregator.py)
MIXIN_OVERRIDES = ("init_model", "deserialize_response", "serialize_response", "create_client_task",
                   "get_test_config", "add_event_handler", "CLIENT_PING", "update_weight_aggregation",
                   "_is_first_result_in_round", "_is_last_result_in_round")
#: methods tests/event_loop.py restates from the reference (its control methods round_completion_handler /
#: event_monitor take test-harness arguments by design and are not compared)
EVENT_LOOP_RESTATED = ("get_client_conf", "create_client_task", "get_test_config", "serialize_response",
                       "deserialize_response", "add_event_handler", "CLIENT_PING", "CLIENT_EXECUTE_COMPLETION",
                       "client_completion_handler")


def params(fn):
    return [(p.name, p.kind.name, None if p.default is inspect.Parameter.empty else repr(p.default))
            for p in inspect.signature(fn).parameters.values()]


def compare(errors, what, mine, ref, allow_extra_defaults=False):
    a, b = params(mine), params(ref)
    if allow_extra_defaults:  # a default where the reference has none is a superset, not a mismatch
        a = [(n, k, d if rb[2] is not None else None) for (n, k, d), rb in zip(a, b)] if len(a) == len(b) else a
    if a != b:
        errors.append(f"{what}: {a} != reference {b}")


#: the AsyncAggregator and AuxoAggregator methods the checks look at
ASYNC_CHECKED = ("create_client_task", "deserialize_response", "serialize_response", "get_test_config", "CLIENT_PING",
                 "update_weight_aggregation")
AUXO_CHECKED = ("update_weight_aggregation", "_is_first_result_in_round", "_is_last_result_in_round")


def live_classes():
    """(Aggregator, AsyncAggregator, AuxoAggregator) imported from the reference checkout."""
    import gen_golden as G

    _, Aggregator, AsyncAggregator, _, _ = G._import_reference()
    # Auxo per-cohort FedAvg (gen_golden.py installs the same placeholders for its off-path modules)
    import types as _t

    nl = _t.ModuleType("nltk")
    nlc = _t.ModuleType("nltk.cluster")
    nlc.KMeansClusterer, nlc.euclidean_distance = object, None
    nl.cluster = nlc
    cfg = _t.ModuleType("config")
    cfg.auxo_config = {}
    sys.modules.update({"nltk": nl, "nltk.cluster": nlc, "config": cfg})
    sys.path.insert(0, os.path.join(G.REF, "examples", "auxo"))
    from aggregator import AuxoAggregator  # examples/auxo/aggregator.py

    return Aggregator, AsyncAggregator, AuxoAggregator


def record(classes) -> dict:
    """{class: {method: {"params": [[name, kind, repr(default) | null], ...], "qualname": ...}}} of the checked methods."""
    Aggregator, AsyncAggregator, AuxoAggregator = classes
    want = ((Aggregator, sorted(set(MIXIN_OVERRIDES + EVENT_LOOP_RESTATED))), (AsyncAggregator, ASYNC_CHECKED),
            (AuxoAggregator, AUXO_CHECKED))
    return {c.__name__: {m: {"params": [list(p) for p in params(getattr(c, m))],
                             "qualname": getattr(c, m).__qualname__} for m in names if hasattr(c, m)}
            for c, names in want}


class _Default:
    """A default value known by its repr alone."""

    def __init__(self, text):
        self.text = text

    def __repr__(self):
        return self.text


def _stand_in(name, methods, bases=()):
    """A class called ``name`` whose own methods are those the record says it defines itself, each with the recorded
    parameter list and ``__qualname__`` (the rest it inherits from ``bases``, as the reference class does)."""
    ns = {}
    for m, r in methods.items():
        if r["qualname"] != f"{name}.{m}":
            continue

        def f(*a, **k):
            raise NotImplementedError("a stand-in for the reference's method")

        f.__name__, f.__qualname__ = m, r["qualname"]
        f.__signature__ = inspect.Signature(
            [inspect.Parameter(n, getattr(inspect.Parameter, kind),
                               default=inspect.Parameter.empty if d is None else _Default(d))
             for n, kind, d in r["params"]])
        ns[m] = f
    return type(name, bases, ns)


def recorded_classes():
    with open(RECORD) as fh:
        rec = json.load(fh)
    for m, r in rec["AsyncAggregator"].items():  # what it inherits must be the base class's own, as recorded there
        if r["qualname"].startswith("Aggregator."):
            assert rec["Aggregator"][m] == r, m
    Aggregator = _stand_in("Aggregator", rec["Aggregator"])
    AsyncAggregator = _stand_in("AsyncAggregator", rec["AsyncAggregator"], (Aggregator,))
    AuxoAggregator = _stand_in("AuxoAggregator", {m: dict(r, qualname="AuxoAggregator." + m)
                                                  for m, r in rec["AuxoAggregator"].items()})
    return Aggregator, AsyncAggregator, AuxoAggregator


def main():
    if "--record" in sys.argv[1:]:
        with open(RECORD, "w") as fh:
            json.dump(record(live_classes()), fh, indent=1, sort_keys=True)
            fh.write("\n")
        print(json.dumps({"ok": True, "recorded": RECORD}))
        return 0
    live = "--live" in sys.argv[1:]
    Aggregator, AsyncAggregator, AuxoAggregator = live_classes() if live else recorded_classes()
    from fedscale_amd.cloud.aggregation import aggregator as M
    from tests import event_loop as EL

    errors, checked = [], []

    class A(M.DeviceAggregatorMixin, Aggregator):
        pass

    a = A.__new__(A)  # no reference __init__ (it opens gRPC and reads the job's data)
    assert A.__mro__[1] is M.DeviceAggregatorMixin and Aggregator in A.__mro__
    for name in MIXIN_OVERRIDES:
        ref = getattr(Aggregator, name, None)
        if ref is None:
            errors.append(f"Aggregator has no {name}")
            continue
        compare(errors, f"DeviceAggregatorMixin.{name}", getattr(M.DeviceAggregatorMixin, name), ref)
        if not a._reference_impl(name):
            errors.append(f"_reference_impl({name!r}) is False over the real Aggregator")
        checked.append(name)
    sup = super(M.DeviceAggregatorMixin, a).init_model
    if getattr(sup, "__qualname__", "") != "Aggregator.init_model":
        errors.append(f"super().init_model is {sup.__qualname__}, not Aggregator.init_model")

    for name in EVENT_LOOP_RESTATED:
        compare(errors, f"tests/event_loop.Aggregator.{name}", getattr(EL.Aggregator, name), getattr(Aggregator, name))

    class E(M.DeviceAggregatorMixin, EL.Aggregator):
        pass

    e = E.__new__(E)
    for name in MIXIN_OVERRIDES:
        if hasattr(EL.Aggregator, name) and not e._reference_impl(name):
            errors.append(f"_reference_impl({name!r}) is False over tests/event_loop.Aggregator")

    class B(M.DeviceAsyncAggregatorMixin, AsyncAggregator):
        pass

    b = B.__new__(B)
    if b._reference_impl("create_client_task"):
        errors.append("FedBuff's create_client_task (async_aggregator.py:40) was not seen as a plugin override")
    for name in ("deserialize_response", "serialize_response", "get_test_config", "CLIENT_PING"):
        if not b._reference_impl(name):
            errors.append(f"_reference_impl({name!r}) is False over AsyncAggregator")
    compare(errors, "DeviceAsyncAggregatorMixin.update_weight_aggregation",
            M.DeviceAsyncAggregatorMixin.update_weight_aggregation, AsyncAggregator.update_weight_aggregation)

    for name in ("update_weight_aggregation", "_is_first_result_in_round", "_is_last_result_in_round"):
        compare(errors, f"DeviceCohortAggregatorMixin.{name}", getattr(M.DeviceCohortAggregatorMixin, name),
                getattr(AuxoAggregator, name), allow_extra_defaults=True)

    report = {"ok": not errors, "against": "the reference checkout" if live else "the recorded signatures",
              "overrides_checked": checked, "event_loop_checked": list(EVENT_LOOP_RESTATED),
              "errors": errors}
    print(json.dumps(report))
    return 0 if not errors else 1


if __name__ == "__main__":
    sys.exit(main())
