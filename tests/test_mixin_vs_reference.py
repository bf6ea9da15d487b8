"""The device mixins composed with the reference Aggregator / AsyncAggregator / AuxoAggregator classes, rebuilt
from the signatures recorded from the real reference (tests/golden/reference_aggregator_signatures.json: every
checked method's parameter list and defining class), so the test needs nothing outside the repository.

The check runs in a child process (tests/golden/check_mixin_vs_reference.py; its --live mode imports the real
classes instead, which needs off-path placeholder modules that must not leak into a test process).  It asserts identical parameter lists for every overridden method, that the MRO hands the
mixin's super() calls to the reference's own methods (``_reference_impl``), that FedBuff's own
create_client_task is left alone, and that tests/event_loop.py restates the reference's signatures."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_mixin_composes_with_the_real_aggregator():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "golden", "check_mixin_vs_reference.py")],
                       cwd=ROOT, capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, PYTHONDONTWRITEBYTECODE="1"))
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert lines, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    report = json.loads(lines[-1])
    assert r.returncode == 0 and report["ok"], report["errors"]
    assert report["against"] == "the recorded signatures"
    assert "update_weight_aggregation" in report["overrides_checked"] and len(report["overrides_checked"]) >= 10
