"""The issue order of one iteration -- every launch with its stream, grouped region and lane, every stream wait and event record
(tests/issue_trace.py) -- against tests/golden/issue_order_parent.txt, the records of the commit before the executor's and the training
step's schedules were rewritten as plain functions over engine.pass_schedule.

The fixture is NEVER regenerated from the code under test.  A pull request that means to change the schedule (which pass forks, what is
grouped, where a join sits) replaces the fixture with the records of its own tree (`python -m tests.issue_trace DIR`, DIR/summary.txt)
and says why, with the whole-iteration A/B that DESIGN.md section 5 ("Issue order") asks for."""
import os

import pytest

pytestmark = pytest.mark.gpu

from tests import issue_trace


@pytest.fixture(scope="module")
def parent(golden_dir):
    return issue_trace.parse_summary(os.path.join(golden_dir, "issue_order_parent.txt"))


def test_fixture_lists_every_case(parent):
    assert sorted(parent) == sorted(issue_trace.CASES)


@pytest.mark.parametrize("case", list(issue_trace.CASES))
def test_issue_order_is_the_parents(case, parent, tmp_path):
    text = issue_trace.record_case(case)
    got_sha, got = issue_trace.parse_summary_line(issue_trace.summary_line(case, text))
    want_sha, want = parent[case]
    print(issue_trace.summary_line(case, text))
    if (got_sha, got) != (want_sha, want):
        path = tmp_path / (case + ".txt")
        path.write_text(text)
        pytest.fail("issue order of %s moved: counts %s (fixture %s), sha256 %s (fixture %s); full record: %s"
                    % (case, got, want, got_sha, want_sha, path))
    if case in ("2d_captured", "3d_captured"):
        # the captured default step does run its non-forking passes (pass B, the early VAT pass, pass A) with grouped launches
        assert int(got["regions"]) > 0 and got["regions"] == want["regions"]
