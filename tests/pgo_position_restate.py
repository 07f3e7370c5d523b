"""tests/pgo_restate.py with position factors (DESIGN.md §2 "Pose graph": pgo_node's gtsam::GPSFactor under useGPS).

A position factor (node, z, var[3], k): residual r = t_node - z (the translation of X_node less the measured point, GTSAM's
GPSFactor::evaluateError), whitened by 1/sqrt(var), Cauchy weight and cost exactly as for a between factor (k == 0:
Gaussian).  Under X <- X Exp(d) with tangent order [w v] its Jacobian is [0 R_node].  The rows of the position factors
follow those of the prior and the between factors in the whitened system; with no position factor every method returns
what pgo_restate.Graph returns, bit for bit.
"""
import numpy as np

import pgo_restate as R


class Graph(R.Graph):
    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.pnode, self.pz, self.pvar, self.pk = [], [], [], []

    def add_position(self, node, xyz, var, robust_k=1.0):
        if not 0 <= node < len(self.init):
            raise ValueError("bad node")
        self.pnode.append(int(node))
        self.pz.append(np.array(xyz, np.float64).reshape(3))
        self.pvar.append(np.broadcast_to(np.asarray(var, np.float64), (3,)).copy())
        self.pk.append(float(robust_k))

    def _parrays(self):
        return np.array(self.pnode, int), np.array(self.pz).reshape(-1, 3), np.array(self.pvar).reshape(-1, 3), np.array(self.pk)

    # ---------------------------------------------------------------------------------------------- evaluation
    def position_residuals(self, poses):
        """(p, 3) unwhitened."""
        X = np.asarray(poses, np.float64)
        node, z, _, _ = self._parrays()
        return X[node, :3, 3] - z

    def _probust(self, r):
        _, _, var, k = self._parrays()
        s = np.sum(r * r / var, -1) if len(r) else np.zeros(0)
        k2 = np.where(k > 0, k * k, 1.0)
        w = np.where(k > 0, k2 / (k2 + s), 1.0)
        rho = np.where(k > 0, 0.5 * k2 * np.log1p(s / k2), 0.5 * s)
        return s, w, rho

    def position_weights(self, poses):
        """The robust weight of every position factor, in the order they were added."""
        return self._probust(self.position_residuals(poses))[1]

    def cost(self, poses):
        c = super().cost(poses)
        if self.pnode:
            c = float(c + np.sum(self._probust(self.position_residuals(poses))[2]))
        return c

    def position_jacobian(self, poses):
        """(p, 3, 6) dr/dd_node = [0 R_node], unwhitened."""
        X = np.asarray(poses, np.float64)
        J = np.zeros((len(self.pnode), 3, 6))
        J[:, :, 3:] = X[np.array(self.pnode, int), :3, :3]
        return J

    def linearize_positions(self, poses):
        """Row blocks of the position factors in the whitened, weighted system: (rows (p, 3), J (p, 3, 6), node)."""
        node, _, var, _ = self._parrays()
        r = self.position_residuals(poses)
        scale = np.sqrt(self._probust(r)[1])[:, None] / np.sqrt(var)
        return r * scale, self.position_jacobian(poses) * scale[..., None], node

    def gn_step_at(self, poses, solver="lstsq"):
        """The Gauss-Newton step (n, 6) of the reweighted problem linearised at poses."""
        n = len(poses)
        r, Ji, Jj, i, j = self.linearize(poses)
        rp, Jp, node = self.linearize_positions(poses)
        m, p = len(r), len(rp)
        rhs = np.concatenate([r.reshape(-1), rp.reshape(-1)])
        if solver == "lstsq":
            A = np.zeros((m, 6, n, 6))
            A[np.arange(m), :, j, :] = Jj
            A[np.arange(1, m), :, i[1:], :] = Ji[1:]
            A = A.reshape(6 * m, 6 * n)
            if p:
                B = np.zeros((p, 3, n, 6))
                B[np.arange(p), :, node, :] = Jp
                A = np.concatenate([A, B.reshape(3 * p, 6 * n)], 0)
            d = np.linalg.lstsq(A, -rhs, rcond=None)[0]
        elif solver == "sparse":
            import scipy.sparse as sp
            import scipy.sparse.linalg as spl
            rows = (6 * np.arange(m)[:, None, None] + np.arange(6)[None, :, None]) + np.zeros((1, 1, 6), int)
            colj = (6 * j[:, None, None] + np.arange(6)[None, None, :]) + np.zeros((1, 6, 1), int)
            coli = (6 * i[1:, None, None] + np.arange(6)[None, None, :]) + np.zeros((1, 6, 1), int)
            prow = (6 * m + 3 * np.arange(p)[:, None, None] + np.arange(3)[None, :, None]) + np.zeros((1, 1, 6), int)
            pcol = (6 * node[:, None, None] + np.arange(6)[None, None, :]) + np.zeros((1, 3, 1), int)
            A = sp.csr_matrix((np.concatenate([Jj.ravel(), Ji[1:].ravel(), Jp.ravel()]),
                               (np.concatenate([rows.ravel(), rows[1:].ravel(), prow.ravel()]),
                                np.concatenate([colj.ravel(), coli.ravel(), pcol.ravel()]))),
                              shape=(6 * m + 3 * p, 6 * n))
            d = spl.spsolve((A.T @ A).tocsc(), -(A.T @ rhs))
        else:
            raise ValueError(solver)
        return d.reshape(n, 6)

    def optimize(self, *a, **kw):
        """pgo_restate.Graph.optimize (it calls cost and gn_step_at above); info gains "position_weights"."""
        X, info = super().optimize(*a, **kw)
        info["position_weights"] = self.position_weights(X)
        return X, info


def build(poses, loops, positions=(), **kw):
    """A Graph of 4x4 poses, loops [(i, j, Z, var, k)] and positions [(node, xyz, var, k)]."""
    g = Graph(**kw)
    for P in poses:
        g.add_node(P)
    for i, j, Z, var, k in loops:
        g.add_between(i, j, Z, var, k)
    for node, xyz, var, k in positions:
        g.add_position(node, xyz, var, k)
    return g
