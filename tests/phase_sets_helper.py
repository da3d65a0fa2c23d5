"""Order loop of a column whose aerosol zones have DIFFERENT phase functions, from the oracle's own pieces (test
infrastructure, not product code).

The oracle's Column holds one (P0_aer, P_aer).  The first order and the source function are linear in the phase data, so for a
column whose aerosol zones j = 0..k-1 use the phase data (P0_j, P_j):

    first order      = first_order(column with alb_aer = 0 in every zone)
                       + sum_j first_order(column with alb_atm = 0, alb_aer = 0 in all aerosol zones but j, P0_aer = P0_j)
    source function  = the same sum of source_function(., In_1) with P_aer = P_j

and transport and the convergence test do not read phase data at all: oracle.transport(c, Jn), oracle.convergence_ratio, in
the loop of oracle.solve_column.  With every zone on the same phase data the sums re-associate the reference's, so the result
agrees with oracle.solve_column to rounding (1e-13 of the field maximum), not to the bit."""
from dataclasses import replace

import numpy as np

import sos_oracle as O


def _parts(c, zone_phase):
    """The columns of the superposition: molecules only, then one per aerosol zone.  `zone_phase`: (P0_aer, P_aer) per aerosol
    zone of `c`, top to bottom."""
    assert c.zone_table is not None, "a column made by make_column_slabs"
    mix = [i for i, z in enumerate(c.zone_table) if z.kind == "mix"]
    assert len(mix) == len(zone_phase)

    def table(keep):
        return [replace(z, alb_aer=(z.alb_aer if i == keep else 0.0)) if z.kind == "mix" else replace(z)
                for i, z in enumerate(c.zone_table)]

    parts = [replace(c, alb_aer=0.0, zone_table=table(-1))]
    for i, (P0, P) in zip(mix, zone_phase):
        parts.append(replace(c, alb_atm=0.0, alb_aer=(c.alb_aer if i == mix[0] else 0.0), zone_table=table(i), P0_aer=P0, P_aer=P))
    return parts


def solve_column_zone_sets(c, zone_phase, tol=1e-4, max_orders=10000, literal=False):
    """oracle.solve_column for a column whose aerosol zone j reads zone_phase[j] = (P0_aer, P_aer)."""
    parts = _parts(c, zone_phase)
    I1 = sum(O.first_order(p) for p in parts)
    In_1 = I1
    I = I1.copy()
    In = np.ones_like(I1)
    n = 1
    while True:
        r = O.convergence_ratio(In, I, c.N)
        if not (r >= tol) or n >= max_orders:
            break
        n += 1
        Jn = sum(O.source_function(p, In_1) for p in parts)
        In = O.transport(c, Jn, literal=literal)
        In_1 = In
        I = I + In
    return O.Solution(I=I, I_saved=np.zeros((0,)), n=n)
