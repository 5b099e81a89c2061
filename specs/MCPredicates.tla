------------------------- MODULE MCPredicates -------------------------
\* User-defined state predicates for the MI355X checker, in its predicate
\* language (DESIGN.md section 13): load with `-predicates` and name a
\* definition under INVARIANT, as one adds an operator to MC.tla for TLC.
\* A file holds at most eight definitions.
\*
\* The first five restate the built-in invariants of specs/MC.tla under names
\* of their own (a built-in's name is refused).  The language has no SubSeq:
\* an equality of prefixes is spelled entry by entry.
EXTENDS MC

PNoTwoLeaders == \A i, j \in Server :
                    (state[i] = Leader /\ state[j] = Leader) => i = j

PElectionSafety == \A e, f \in elections : e.eterm = f.eterm => e.eleader = f.eleader

PLogMatching == \A i, j \in Server :
                  \A n \in 1..Min(Len(log[i]), Len(log[j])) :
                     log[i][n].term = log[j][n].term =>
                         \A k \in 1..n : log[i][k] = log[j][k]

PStateMachineSafety == \A i, j \in Server :
    \A n \in 1..Min(commitIndex[i], commitIndex[j]) :
        (n <= Len(log[i]) /\ n <= Len(log[j])) => log[i][n] = log[j][n]

PLeaderCompleteness == \A i, j \in Server :
    (state[i] = Leader /\ currentTerm[j] <= currentTerm[i]) =>
        \A n \in 1..commitIndex[j] :
            n <= Len(log[j]) => (n <= Len(log[i]) /\ log[i][n] = log[j][n])

(* The witness idiom: to FIND a state, assert its negation and read the trace.
   This one is violated by the first state in which a leader has committed. *)
NoCommit == ~ \E i \in Server : state[i] = Leader /\ commitIndex[i] >= 1

\* A vote counted in the voter's current term is the vote the voter remembers.
GrantedVotesAreRemembered == \A i, j \in Server :
    (j \in votesGranted[i] /\ currentTerm[i] = currentTerm[j]) => votedFor[j] = i

\* No message carries a term ahead of its sender's.
MessagesWithinSenderTerm == \A m \in DOMAIN messages : m.mterm <= currentTerm[m.msource]
=======================================================================
