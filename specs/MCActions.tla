--------------------------- MODULE MCActions ---------------------------
\* Action properties for the MI355X checker (DESIGN.md section 14): load with
\* `-predicates` and name a definition under PROPERTY, as one does for TLC.
\* An action definition is `Name == [][A]_vars`: A is a predicate over a step,
\* in which a primed variable reads the successor state.  It must hold on
\* every step that changes the state; a stuttering step satisfies it.
\* A file holds at most eight action definitions.
EXTENDS MC

\* ---- laws of raft.tla: they hold on every step

\* The fifth safety property of the Raft paper (Leader Append-Only): a server
\* that stays leader of the same term never overwrites or deletes an entry.
LeaderAppendOnly == [][ \A i \in Server :
    (state[i] = Leader /\ state'[i] = Leader /\ currentTerm'[i] = currentTerm[i])
      => (Len(log'[i]) >= Len(log[i]) /\ \A n \in 1..Len(log[i]) : log'[i][n] = log[i][n]) ]_vars

TermsNeverDecrease == [][ \A i \in Server : currentTerm'[i] >= currentTerm[i] ]_vars

\* Within a term a vote, once cast, is kept (Restart keeps votedFor too).
OneVotePerTerm == [][ \A i \in Server :
    (currentTerm'[i] = currentTerm[i] /\ votedFor[i] # Nil) => votedFor'[i] = votedFor[i] ]_vars

\* A step sends, receives, duplicates or drops at most one copy of a message.
BagChangesByOne == [][ BagCardinality(messages') <= BagCardinality(messages) + 1
                       /\ BagCardinality(messages) <= BagCardinality(messages') + 1 ]_vars

\* elections is a history variable: a step adds at most one record, never removes one.
ElectionsGrow == [][ Cardinality(elections') >= Cardinality(elections)
                     /\ Cardinality(elections') <= Cardinality(elections) + 1 ]_vars

\* ---- witnesses: each is violated, and the trace ends in the step that does it

\* Violated by the first Restart of a leader.
LeadersStay == [][ \A i \in Server : state[i] = Leader => state'[i] = Leader ]_vars

\* raft.tla resets commitIndex on Restart: violated by the first Restart of a
\* server that has committed an entry.
CommitNeverDecreases == [][ \A i \in Server : commitIndex'[i] >= commitIndex[i] ]_vars

\* Violated by the first Timeout.
TermsFrozen == [][ \A i \in Server : currentTerm'[i] = currentTerm[i] ]_vars
=======================================================================
