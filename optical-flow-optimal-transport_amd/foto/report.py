"""The transport report: what foto_bb_report (include/foto.h) sums per time plane, and the scalars
a caller derives from it on the host.

The table is ``(Nt, 8)`` float64, one row per time plane; the columns are the FOTO_REPORT_*
indices of the header.  Every derived value is one numpy expression over the table, so a caller
who wants another combination can write it the same way.
"""
import numpy as np

REPORT_COLS = 8
# column name -> index (include/foto.h FOTO_REPORT_*)
COLUMNS = {"MASS": 0, "KINETIC": 1, "VACUUM": 2, "CONT": 3, "HJ_NUM": 4, "HJ_DEN": 5, "DUAL": 6, "DIST_T": 7}
MASS, KINETIC, VACUUM, CONT, HJ_NUM, HJ_DEN, DUAL, DIST_T = range(REPORT_COLS)


class TransportReport:
    """An immutable record of one report: ``table`` (Nt, 8) float64 (read-only), ``Nt``, ``Nx``,
    ``Ny``.  One array view per column (``mass``, ``kinetic``, ``vacuum``, ``cont``, ``hj_num``,
    ``hj_den``, ``dual``, ``dist_t``: each (Nt,)), and the derived values below."""

    __slots__ = ("table", "Nt", "Nx", "Ny")

    def __init__(self, table, Nt, Nx, Ny):
        Nt, Nx, Ny = int(Nt), int(Nx), int(Ny)
        t = np.array(table, dtype=np.float64).reshape(-1)
        if t.size != Nt * REPORT_COLS:
            raise ValueError(f"table of {t.size} values; a report of Nt = {Nt} planes has {Nt * REPORT_COLS}")
        t = t.reshape(Nt, REPORT_COLS)
        t.setflags(write=False)
        for name, v in (("table", t), ("Nt", Nt), ("Nx", Nx), ("Ny", Ny)):
            object.__setattr__(self, name, v)

    def __setattr__(self, name, value):
        raise AttributeError("TransportReport is immutable")

    def __delattr__(self, name):
        raise AttributeError("TransportReport is immutable")

    # ------------------------------------------------------------------ columns
    mass = property(lambda self: self.table[:, MASS])
    kinetic = property(lambda self: self.table[:, KINETIC])
    vacuum = property(lambda self: self.table[:, VACUUM])
    cont = property(lambda self: self.table[:, CONT])
    hj_num = property(lambda self: self.table[:, HJ_NUM])
    hj_den = property(lambda self: self.table[:, HJ_DEN])
    dual = property(lambda self: self.table[:, DUAL])
    dist_t = property(lambda self: self.table[:, DIST_T])

    # ------------------------------------------------------------------ derived
    @property
    def crit(self):
        """The solver's convergence criterion of that iteration (benamou_brenier.py:246-249), up
        to summation order."""
        return float(np.sqrt(np.sum(self.hj_num) / (np.sum(self.hj_den) + 1e-10)))

    @property
    def action(self):
        """The Benamou-Brenier action, primal: the trapezoid of KINETIC over n = 0..Nt-1, dt = 1."""
        return float(np.sum(0.5 * (self.kinetic[1:] + self.kinetic[:-1])))

    @property
    def action_dual(self):
        """The dual estimate of the same action, sum phi_{Nt-1} rhoT - sum phi_0 rho0.  It agrees
        with ``action`` only at convergence and for equal masses."""
        return float(np.sum(self.dual))

    @property
    def w2(self):
        """The W2 estimate sqrt(2 (Nt-1) action): the path takes Nt-1 time units."""
        return float(np.sqrt(2.0 * (self.Nt - 1) * self.action))

    @property
    def w2_dual(self):
        """sqrt(2 (Nt-1) action_dual); NaN when action_dual is negative."""
        a = self.action_dual
        return float(np.sqrt(2.0 * (self.Nt - 1) * a)) if a >= 0 else float("nan")

    @property
    def ie(self):
        """utils.IE(Nx, Ny, rhoT, rho_n) of every plane (benamou_brenier.py:265): (Nt,)."""
        return 255.0 * np.sqrt(self.dist_t / (self.Nx * self.Ny))

    @property
    def continuity(self):
        """The 2-norm of the continuity residual with its two boundary frames."""
        return float(np.sqrt(np.sum(self.cont)))

    @property
    def mass_drift(self):
        """Largest minus smallest plane mass: zero when mass is conserved along the path."""
        return float(self.mass.max() - self.mass.min())

    def __repr__(self):
        return (f"TransportReport(Nt={self.Nt}, Nx={self.Nx}, Ny={self.Ny}, crit={self.crit:.6g}, "
                f"action={self.action:.6g}, action_dual={self.action_dual:.6g}, continuity={self.continuity:.3g}, "
                f"mass_drift={self.mass_drift:.3g})")
