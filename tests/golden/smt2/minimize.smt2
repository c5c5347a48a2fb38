; a minimising query: classified, never searched
(declare-fun |1_calldatasize| () (_ BitVec 256))
(declare-fun call_value1 () (_ BitVec 256))
(assert (bvuge |1_calldatasize| (_ bv4 256)))
(assert (bvult call_value1 #x0000000000000000000000000000000000000000000000000de0b6b3a7640000))
(minimize |1_calldatasize|)
(minimize call_value1)
(check-sat)
