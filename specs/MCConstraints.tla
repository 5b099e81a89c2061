------------------------- MODULE MCConstraints -------------------------
\* User-defined CONSTRAINTs for the MI355X checker, in its predicate language
\* (DESIGN.md sections 13 and 16): load with `-predicates` and name a
\* definition under CONSTRAINT beside StateConstraint, as one adds an operator
\* to MC.tla for TLC.  A state on which a named definition is FALSE is checked
\* against the invariants, then neither counted nor expanded.
\*
\* Under SYMMETRY a constraint must treat the servers alike, as TLC requires;
\* every definition below does.  The language has no constants of the model:
\* a bound is a number.
EXTENDS MC

\* The four bounds of StateConstraint (specs/MC.tla) restated, each tighter
\* than a cfg may set it: with MaxTerm = 3 in the cfg, TermsUpTo2 gives the
\* state space of MaxTerm = 2.
TermsUpTo2 == \A i \in Server : currentTerm[i] <= 2

LogsUpTo1 == \A i \in Server : Len(log[i]) <= 1

CopiesUpTo1 == \A m \in DOMAIN messages : messages[m] <= 1

InFlightUpTo1 == BagCardinality(messages) <= 1

\* Shapes no bound gives.  At most one candidate at a time:
OneCandidate == \A i, j \in Server :
                   (state[i] = Candidate /\ state[j] = Candidate) => i = j

\* no more than one election won:
OneElection == Cardinality(elections) <= 1

\* nobody commits:
NobodyCommits == \A i \in Server : commitIndex[i] = 0
=======================================================================
