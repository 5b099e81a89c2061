"""The command line's text code (raft-tla_amd/csrc/rtla_cli_text.h: cfg grammar, the definitions of a predicate
file, name substitution, sha256) as a stand-alone program under the address and undefined-behaviour sanitizers:
host code only, no device and no library.  Well-formed inputs print what was parsed; hostile ones must end clean."""
import os
import shutil
import subprocess

import pytest

from cli_util import ROOT, model_dir

SPECS = os.path.join(ROOT, "specs")
HOSTILE = {
    "unterminated_string.cfg": 'CONSTANTS\n    Leader = "Lead',
    "lone_quote.cfg": 'CONSTANT Nil = "',
    "unterminated_comment.tla": "P == TRUE\n(* never closed (* nested\nQ == FALSE\n",
    "constant_at_eof.cfg": "SPECIFICATION Spec\nCONSTANT X =",
    "constant_arrow_at_eof.cfg": "CONSTANT X <-",
    "open_brace.cfg": "CONSTANT Server = {r1, r2",
    "empty.tla": "",
    "name_at_end.tla": "P == s1 = v1 /\\ xs1 # \"s1\" /\\ s12 /\\ s3 /\\ s2",
    "equals_at_end.tla": "P ==",
    "name_then_blanks.tla": "Name   \t ",
    "comment_opens_at_end.tla": "P == TRUE (*",
    "line_comment_at_end.tla": "P == [][ TRUE ]_vars \\*",
    "rule_in_definition.tla": "A == [][\nB == 1\n====\nC == 2\n",
}
NAMES = {
    "MCPredicates.tla": ("[PNoTwoLeaders,PElectionSafety,PLogMatching,PStateMachineSafety,PLeaderCompleteness,NoCommit,"
                         "GrantedVotesAreRemembered,MessagesWithinSenderTerm]", "[]"),
    "MCActions.tla": ("[]", "[LeaderAppendOnly,TermsNeverDecrease,OneVotePerTerm,BagChangesByOne,ElectionsGrow,"
                      "LeadersStay,CommitNeverDecreases,TermsFrozen]"),
}


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    """The program's output, one block of lines per input file."""
    cxx = shutil.which("g++") or shutil.which("clang++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    tmp = tmp_path_factory.mktemp("cli_text")
    exe = str(tmp / "cli_text")
    flags = [cxx, "-std=c++20", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    (tmp / "probe.cpp").write_text("int main() { return 0; }\n")
    if subprocess.run(flags + [str(tmp / "probe.cpp"), "-o", str(tmp / "probe")], capture_output=True).returncode != 0:
        pytest.skip("the compiler has no sanitizer runtime")  # (an empty program does not link: no error of ours)
    build = subprocess.run(flags + ["-I", os.path.join(ROOT, "raft-tla_amd", "csrc"),
                                    os.path.join(ROOT, "tests", "cli_text_main.cpp"), "-o", exe],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    _, cfg = model_dir(str(tmp / "model"), 3, 2, 2, 1, 1, 1, ["NoTwoLeaders", "LogMatching"], symmetry=True,
                       extra="PROPERTIES A B \\* a comment\n(* and (* another *)\nCONSTRAINTS C\nCHECK_DEADLOCK FALSE\n")
    files = [cfg] + sorted(os.path.join(SPECS, f) for f in os.listdir(SPECS) if f.endswith(".tla"))
    for name, text in HOSTILE.items():
        (tmp / name).write_text(text)
        files.append(str(tmp / name))
    run = subprocess.run([exe] + files, capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    assert run.stderr == "" and run.stdout.endswith("\nok\n")
    assert "sha256(abc) = ba7816bf8f01cfea414140de5dae2223b00361a396177a9cb410ff61f20015ad\n" in run.stdout
    blocks = {}
    for block in run.stdout.split("\n@@ ")[1:]:
        blocks[block.split(":")[0]] = block.split("\n")[1:]
    assert set(blocks) == {"MC.cfg"} | {os.path.basename(f) for f in files[1:]}
    return blocks


def test_a_cfg_is_parsed_into_its_parts(report):
    assert report["MC.cfg"][0] == (
        'cfg: spec=Spec sym=Perms inv=[NoTwoLeaders,LogMatching] cons=[StateConstraint,C] PROPERTIES=[A,B]'
        ' Server=[r1,r2,r3] Value=[x1,x2]'
        ' AppendEntriesRequest="AppendEntriesRequest" AppendEntriesResponse="AppendEntriesResponse"'
        ' Candidate="Candidate" Follower="Follower" Leader="Leader" MaxCopies=1 MaxInFlight=1 MaxLogLen=1 MaxTerm=2'
        ' Nil="Nil" RequestVoteRequest="RequestVoteRequest" RequestVoteResponse="RequestVoteResponse"')


def test_the_definitions_of_the_spec_files(report):
    for name, (states, actions) in NAMES.items():
        assert report[name][1].startswith("defs: states=%s actions=%s end=" % (states, actions)), report[name][1]
        # every other one of the eight kept; a selection of states keeps no action definition, whatever was named
        assert report[name][2].endswith(" 4 definitions left")
        assert report[name][3].endswith(" %d definitions left" % (0 if actions != "[]" else 4))
    # MC.tla's operators are state definitions; a module's text is no cfg
    assert "NoTwoLeaders,ElectionSafety,Perms,LogMatching" in report["MC.tla"][1] and "actions=[]" in report["MC.tla"][1]
    assert report["MC.tla"][0].startswith("cfg error: ")
    for name in ("TermsUpTo2", "InFlightUpTo1", "OneCandidate", "NobodyCommits"):
        assert name in report["MCConstraints.tla"][1]


def test_hostile_inputs_end_clean_and_say_what_they_are(report):
    assert report["unterminated_string.cfg"][0] == 'cfg: spec= sym= inv=[] cons=[] =[] Leader="Lead'
    assert report["lone_quote.cfg"][0] == 'cfg: spec= sym= inv=[] cons=[] =[] Nil="'
    assert report["constant_at_eof.cfg"][0] == "cfg error: bad CONSTANT near 'X'"
    assert report["constant_arrow_at_eof.cfg"][0] == "cfg error: bad CONSTANT near 'X'"
    assert report["open_brace.cfg"][0] == "cfg: spec= sym= inv=[] cons=[] =[] Server=[r1,r2]"
    assert report["empty.tla"][:2] == ["cfg: spec= sym= inv=[] cons=[] =[]", "defs: states=[] actions=[] end=0"]
    assert report["unterminated_comment.tla"][1] == "defs: states=[P] actions=[] end=47"
    assert report["equals_at_end.tla"][1] == "defs: states=[P] actions=[] end=4"
    assert report["name_then_blanks.tla"][1] == "defs: states=[] actions=[] end=9"
    assert report["comment_opens_at_end.tla"][1] == "defs: states=[P] actions=[] end=12"
    assert report["line_comment_at_end.tla"][1] == "defs: states=[] actions=[P] end=23"
    # a definition ends where the next one starts, the module where its closing rule does
    assert report["rule_in_definition.tla"][1] == "defs: states=[B] actions=[A] end=16"
    # (blanked: the characters that were no blank before; `B == 1` has four, `A == [][` six more)
    assert report["rule_in_definition.tla"][2] == "select([A], states_only=0): 4 blanked, 1 definitions left"
    assert report["rule_in_definition.tla"][3] == "select([A], states_only=1): 10 blanked, 0 definitions left"
    # s1 / v1 are the row printer's names; inside a longer name, a string, or past the model's size they stay
    assert report["name_at_end.tla"][4] == 'subst: P == r1 = x1 /\\ xs1 # "s1" /\\ s12 /\\ s3 /\\ r2'
