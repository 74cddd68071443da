"""
lbfgs.py - limited-memory BFGS with an Armijo backtracking line search, written as a state
machine that consumes one (params, error, grads) triple per evaluation and returns the next trial
parameters. That is the shape the lock-step multi-start drivers need (core/batch.py): B seeds
advance one evaluation at a time, each with its own state. LBFGSB (SciPy's minimize) owns its loop
and stays single-seed.

One evaluation is either accepted (Armijo: error <= f + armijo * g.(p - x)) - the pair
(s, y) = (p - x, grads - g) enters the history if its curvature is safely positive, and the next
direction comes from the two-loop recursion with a unit first step - or rejected, and the step
shrinks. When a quasi-Newton direction runs out of backtracks the history is dropped and the seed
restarts along -g with the step first_step / |g|; when a steepest-descent direction runs out of
backtracks the seed is `finished`: it returns to its last accepted point and takes no further steps.

Every product and sum is rounded on its own and every inner product is accumulated in ONE defined
order (dot(), below), which qocx_lbfgs.hip reproduces: the device-resident route of the multi-start
drivers walks this file's trajectory bit for bit.
"""

import numpy as np

LANES = 256
# a pair (s, y) is stored iff s.y > 0 and (s.y)^2 > CURVATURE_FLOOR (s.s) (y.y)
CURVATURE_FLOOR = 1e-20


def dot(a, b):
    """a.b in the order of the device kernel: lane l of 256 accumulates the elements l, l + 256,
    l + 512, ... in increasing index as acc = acc + a[i] * b[i] (two roundings), then the 256
    partial sums are folded by the tree partial[l] += partial[l + stride], stride = 128 .. 1."""
    count = a.size
    rows = -(-count // LANES)
    products = np.zeros(rows * LANES)  # (acc + 0.0 leaves acc as it is: the padding is exact)
    np.multiply(a, b, out=products[:count])
    products = products.reshape(rows, LANES)
    acc = np.zeros(LANES)
    for row in products:
        acc = acc + row
    stride = LANES // 2
    while stride:
        acc[:stride] = acc[:stride] + acc[stride:2 * stride]
        stride //= 2
    return acc[0]


class LBFGS(object):
    """LBFGS(history=10, first_step=1.0, armijo=1e-4, shrink=0.5, max_backtracks=20).

    history: pairs (s, y) kept; first_step: length of the first trial step along -g after a
    (re)start; armijo: sufficient-decrease constant; shrink: factor of a backtrack;
    max_backtracks: rejected trials a direction may take before the restart / the finish.

    update(grads, params, error) -> next trial parameters, where (params, error, grads) is the
    evaluation just made. `finished` is set once a steepest-descent direction has exhausted its
    backtracks; from then on update() returns the last accepted point and changes nothing.
    """

    name = "lbfgs"
    needs_error = True  # the multi-start drivers pass the seed's error to update()

    def __init__(self, history=10, first_step=1.0, armijo=1e-4, shrink=0.5, max_backtracks=20):
        super().__init__()
        if int(history) < 1:
            raise ValueError("history must be >= 1")
        self.history = int(history)
        self.first_step = float(first_step)
        self.armijo = float(armijo)
        self.shrink = float(shrink)
        self.max_backtracks = int(max_backtracks)
        self.reset()

    def __str__(self):
        return ("{}, history: {}, first_step: {}, armijo: {}, shrink: {}, max_backtracks: {}"
                "".format(self.name, self.history, self.first_step, self.armijo, self.shrink,
                          self.max_backtracks))

    def reset(self):
        """Fresh state: the next update() is a seed's first call."""
        self.x = self.f = self.g = self.d = None
        self.t = 0.0
        self.bt = 0
        self.steepest = True
        self.pairs = []  # (s, y, rho), oldest first
        self.gamma = 1.0  # s.y / y.y of the newest stored pair
        self.finished = False
        # counters for the curious (and the tests): not part of the arithmetic
        self.restarts = 0
        self.skipped_pairs = 0
        self.accepted = 0

    def _restart(self):
        self.pairs = []
        self.d = -self.g
        self.steepest = True
        self.bt = 0
        gg = dot(self.g, self.g)
        self.t = self.first_step / np.sqrt(gg) if gg != 0 else 0.0
        self.restarts += 1

    def _two_loop(self):
        """-H g by the two-loop recursion over the stored pairs."""
        q = self.g.copy()
        alphas = []
        for s, y, rho in reversed(self.pairs):  # newest to oldest
            alpha = rho * dot(s, q)
            q = q - alpha * y
            alphas.append(alpha)
        q = q * self.gamma
        for (s, y, rho), alpha in zip(self.pairs, reversed(alphas)):  # oldest to newest
            beta = rho * dot(y, q)
            q = q + (alpha - beta) * s
        return -q

    def update(self, grads, params, error):
        if self.finished:
            return self.x.copy()
        p = np.array(params, dtype=np.float64)
        gp = np.array(grads, dtype=np.float64)
        fp = float(error)
        if self.x is None:  # the first call of a seed: accepted unconditionally
            self.x, self.f, self.g = p, fp, gp
            self.accepted += 1
            self._restart()
            return self.x + self.t * self.d
        step = p - self.x
        if not fp <= self.f + self.armijo * dot(self.g, step):  # (a NaN error rejects)
            self.bt += 1
            self.t = self.t * self.shrink
            if self.bt > self.max_backtracks:
                if self.steepest:
                    self.finished = True
                    return self.x.copy()
                self._restart()
            return self.x + self.t * self.d
        y = gp - self.g
        sy, ss, yy = dot(step, y), dot(step, step), dot(y, y)
        if sy > 0 and sy * sy > CURVATURE_FLOOR * ss * yy:
            self.pairs.append((step, y, 1.0 / sy))
            self.gamma = sy / yy
            if len(self.pairs) > self.history:
                self.pairs.pop(0)
        else:
            self.skipped_pairs += 1
        self.x, self.f, self.g = p, fp, gp
        self.accepted += 1
        if not self.pairs:
            self._restart()
        else:
            self.d = self._two_loop()
            self.t = 1.0
            self.bt = 0
            self.steepest = False
            if not dot(self.g, self.d) < 0:
                self._restart()
        return self.x + self.t * self.d

    def run(self, function, iteration_count, initial_params, jacobian, args=()):
        """The single-seed loop. Like LBFGSB it calls BOTH `jacobian` (gradients; the drivers'
        best-so-far bookkeeping and logging live there) and `function` (the error) once per
        iteration, so an iteration costs two evaluations of the caller's problem. Stops at a
        terminate flag of either, or when the optimizer is finished."""
        self.reset()
        params = initial_params
        for _ in range(iteration_count):
            grads, terminate = jacobian(params, *args)
            if terminate:
                break
            error, terminate = function(params, *args)
            if terminate:
                break
            params = self.update(grads, params, error)
            if self.finished:
                break
        return params
