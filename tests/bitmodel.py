"""An unpacked model of the four operations every GPU test leans on, to pin the oracle at the state widths
no reference golden reaches (``test_shape_sweep_host.py``).

Deliberately plain: a state is a Python list of N ints (0/1), a batch a list of such lists. There are no
64-bit state words, no tail masks and no shifts by a node index anywhere -- the places where the word-packed
oracle (``oracle/pbn_oracle.c``) and the kernels could share a mistake at ``N % 64 == 0``, at a word boundary or
at a new ``W``. Written from DESIGN.md (§4 "RNG modes": streams, counters, node and choice words; §3/§4:
integer thresholds) and the comments of ``include/pbn_abi.h``, not from the oracle's code:

* ``init_philox``       -- ``pbn_randomize_state``: fair bits, truth-table networks clear node 0;
* ``step_philox`` / ``step_forced`` -- ``pbn_step`` / ``pbn_step_forced``, both network kinds;
* ``env_reset_philox``  -- ``pbn_env_reset``: a reset cube drawn uniformly, its '*' bits drawn fair;
* ``env_step_multi``    -- ``pbn_env_step_multi``: flips (dedup, offset, Python list indexing), the
  until-attractor loop with ``first_update_tested`` both ways, cap, horizon, reward and flags.

Draws come from ``oracle.philox4x32_10`` (pinned by Random123's known-answer vectors in ``test_oracle.py``),
the decisions from the network object's *integer* thresholds (``pred_thr`` / ``thr``), where the oracle
compares in fp64 as the reference does -- so the two also disagree if a threshold is off.

Not modelled: the SSD (``orc_ssd_philox``) and synchronous (``orc_sync_philox``) oracle paths, the MT mode and
the replay mode (the last two are pinned by reference goldens directly).
"""

import oracle as O

M32 = 0xFFFFFFFF
STREAM_STEP, STREAM_INIT, STREAM_ENV, STREAM_RESET = 1, 2, 3, 4


def draw(seed, c0, c1, gid, stream):
    """Four 32-bit words: key = the 64-bit seed, counter = {c0, c1, gid_lo, (gid_hi & 0xFFFFFF) | stream << 24}."""
    return O.philox4x32_10([c0 & M32, c1 & M32, gid & M32, ((gid >> 32) & 0xFFFFFF) | (stream << 24)],
                           [seed & M32, (seed >> 32) & M32])


def k53_of_word(a):
    """``random()`` = k53 * 2^-53 from one 32-bit choice word: k53 = a << 21 | a >> 11."""
    return a * (1 << 21) + a // (1 << 11)


def fair_bits(seed, first_call, reset_count, gid, stream, N):
    """Bit stream of the init / reset draws: call ``first_call + m`` yields 128 bits, word 0 first, each word
    from its least significant bit; node i takes bit i of that stream."""
    bits = []
    m = 0
    while len(bits) < N:
        for w in draw(seed, first_call + m, reset_count, gid, stream):
            for _ in range(32):
                bits.append(w % 2)
                w //= 2
        m += 1
    return bits[:N]


class BitModel:
    def __init__(self, net):
        self.N = N = net.n_nodes
        self.kind = net.kind
        self.nodes = []
        if net.kind == 1:
            for i in range(N):
                preds = []
                for j in range(int(net.pred_offsets[i]), int(net.pred_offsets[i + 1])):
                    tt = int(net.pred_tt[j])
                    table = [(tt // (1 << p)) % 2 for p in range(16)]
                    preds.append((int(net.pred_thr[j]), [int(v) for v in net.pred_inputs[j]], table))
                self.nodes.append(preds)
        else:
            for i in range(N):
                ins = [int(v) for v in net.inputs[int(net.input_offsets[i]):int(net.input_offsets[i + 1])]]
                thr = [int(v) for v in net.thr[int(net.thr_offsets[i]):int(net.thr_offsets[i + 1])]]
                self.nodes.append((ins, thr))

    # ---- one node update ------------------------------------------------------------------------------
    def next_value(self, x, i, k53):
        if self.kind == 1:
            # predictor j = min(#{j : k53 >= T_j}, n - 1); output = table[x_in0 x_in1 x_in2 x_self]
            preds = self.nodes[i]
            j = min(sum(1 for thr, _, _ in preds if k53 >= thr), len(preds) - 1)
            _, ins, table = preds[j]
            return table[8 * x[ins[0]] + 4 * x[ins[1]] + 2 * x[ins[2]] + x[i]]
        ins, thr = self.nodes[i]
        idx = 0
        for n in ins:  # C order: the lowest input node is the most significant index bit
            idx = 2 * idx + x[n]
        return 1 if k53 < thr[idx] else 0

    def pick_node(self, w):
        """mulhi(w, N) for the predictor mix (randint(0, N-1)), 1 + mulhi(w, N-1) for tables (randint(1, N-1))."""
        return (w * self.N) // (1 << 32) if self.kind == 1 else 1 + (w * (self.N - 1)) // (1 << 32)

    # ---- state init -----------------------------------------------------------------------------------
    def init_philox(self, B, seed, env_base=0, reset_count=0):
        out = []
        for e in range(B):
            x = fair_bits(seed, 0, reset_count, env_base + e, STREAM_INIT, self.N)
            if self.kind == 2:
                x[0] = 0
            out.append(x)
        return out

    # ---- step modes -----------------------------------------------------------------------------------
    def step_philox(self, bits, seed, env_base, update_base, T, forced=None):
        """Update u of env g: the call keyed by (u, g // 2) -- envs 2m and 2m + 1 share it -- and of its
        words 2(g % 2) (node) and 2(g % 2) + 1 (choice). ``forced[t][e]``: the caller's node instead."""
        out = []
        for e, row in enumerate(bits):
            x = list(row)
            g = env_base + e
            for t in range(T):
                u = update_base + t
                w = draw(seed, u, u >> 32, g // 2, STREAM_STEP)
                node = self.pick_node(w[2 * (g % 2)]) if forced is None else int(forced[t][e])
                x[node] = self.next_value(x, node, k53_of_word(w[2 * (g % 2) + 1]))
            out.append(x)
        return out

    def step_forced(self, bits, node_idx, seed, env_base, update_base):
        return self.step_philox(bits, seed, env_base, update_base, len(node_idx), forced=node_idx)

    # ---- R6 env ---------------------------------------------------------------------------------------
    def env_reset_philox(self, bits, n_steps, reset_cubes, mask=None, seed=0, env_base=0, reset_count=0):
        """Envs with mask[e] != 0: cube = mulhi(word 0 of call 0, n_cubes); fair bits from calls 1, 2, ...;
        the cube's cared nodes take its values; tables clear node 0; n_steps = 0."""
        out, ns = [list(r) for r in bits], list(n_steps)
        for e in range(len(out)):
            if mask is not None and not mask[e]:
                continue
            g = env_base + e
            x = fair_bits(seed, 1, reset_count, g, STREAM_RESET, self.N)
            cube = reset_cubes[(draw(seed, 0, reset_count, g, STREAM_RESET)[0] * len(reset_cubes)) // (1 << 32)]
            for i, c in enumerate(cube):
                if c != "*":
                    x[i] = int(c)
            if self.kind == 2:
                x[0] = 0
            out[e], ns[e] = x, 0
        return out, ns

    @staticmethod
    def _matches(x, cube_items):
        return all(x[i] == v for i, v in cube_items)

    def env_step_multi(self, attractors, horizon, bits, n_steps, actions, dedup=True, offset=1, seed=0, env_base=0,
                       call_idx=0, update_cap=1 << 20, first_tested=False, reward_success=1000, action_cost=1):
        """``attractors``: the reference's ``all_attractors`` (lists of cubes of ints / '*'); attracting = any
        cube matches; target = the last attractor's first cube. Returns a dict of lists like the oracle's."""
        N = self.N
        cubes = [[(i, int(c)) for i, c in enumerate(cube) if c != "*"] for a in attractors for cube in a]
        target = [(i, int(c)) for i, c in enumerate(attractors[-1][0]) if c != "*"]
        for row in actions:  # every env is validated before any state changes
            for a in row:
                if a != 0 and not (-N <= a - offset < N):
                    raise ValueError("action out of range")
        res = dict(state=[], n_steps=[], obs=[], reward=[], flags=[], n_updates=[])
        for e, row in enumerate(bits):
            x = list(row)
            g = env_base + e
            steps = n_steps[e] + 1
            acts = [int(a) for a in actions[e]]
            if dedup:
                acts = sorted(set(acts))  # tensor.unique()
            for a in acts:
                if a != 0:
                    x[a - offset] = 1 - x[a - offset]  # Python list indexing: negative wraps
            obs = list(x)  # the observation is taken before the first update ...
            used, capped = 0, False
            while True:
                if used >= update_cap:
                    capped = True
                    break
                w = draw(seed, used // 2, call_idx, g, STREAM_ENV)
                node = self.pick_node(w[2 * (used % 2)])
                x[node] = self.next_value(x, node, k53_of_word(w[2 * (used % 2) + 1]))
                used += 1
                if used > 1 or first_tested:  # ... and the state after update 1 is not looked at (unless tested)
                    obs = list(x)
                if any(self._matches(obs, c) for c in cubes):
                    break
            term = self._matches(obs, target)
            res["state"].append(x)
            res["n_steps"].append(steps)
            res["obs"].append(obs)
            res["reward"].append((reward_success if term else 0) - action_cost * len(acts))
            res["flags"].append(int(term) + 2 * int(steps == horizon) + 4 * int(capped))
            res["n_updates"].append(used)
        return res
