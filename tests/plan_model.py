"""The documented policy of the detection graph cache (vksift_detect.c: graph_lookup, launch_detection; vksift_instance.c: resize_detect_scratch,
read_switches; vksift_defer.c), restated: which detection launches when, whether it is eligible for replay, its key, eight entries with LRU
eviction, drop-all when the detection scratch is re-allocated or the first describe call extends the descriptor scale table, the permanent
give-up at the 33rd consecutive miss.

The model walks a script of tests/plan_scripts.py and says, per call, what the cache must do: ("capture", exec, evicted exec or None),
("replay", exec), ("drop", [execs]). Execs are numbered in the order of their captures, as the simulated device numbers them. Two facts are
OBSERVATIONS, taken from the log of the same script on a VKSIFT_GRAPH=0 instance (where no graph logic runs): whether a detection ended with the
feature posting (`post`, half of the key) and whether a call re-allocated the scratch for a shape (`grew`). Everything else follows from the
script: deferred submission (sift_buffer_count below VKSIFT_DEFER_CHUNK, so that only full batches and other entry points launch), the capacity
doubling, overlapped batches, profiling, the matcher's cache blocks (`dense`), the input pointer.
"""
GRAPH_CACHE, GIVE_UP_AFTER = 8, 32


def has_octave(w, h, ups):
    return min(w, h) >= (16 if ups else 32)


class Model:
    def __init__(self, script, graph_env=None):
        c, env = script["create"], dict(script["env"])
        if graph_env is not None:
            env["VKSIFT_GRAPH"] = graph_env
        self.c = c
        self.bc, self.nbuf, self.ups = c["bc"], c["nbuf"], c["ups"]
        self.det_cap = self.bc
        g = env.get("VKSIFT_GRAPH")
        self.use_graphs = not (g or "1").startswith("0")
        self.graph_max_pixels = float("inf") if (g or "").startswith("1") else 640 * 480
        pp = env.get("VKSIFT_PYR_PINGPONG")
        self.pingpong = (pp[0] in "12") if pp else self.bc >= 8
        self.pyr_nbuf = 2 if pp and pp[0] == "2" else 1
        self.overlap_forced, self.overlap_min = pp is not None, 1
        self.defer_max = min(int(env.get("VKSIFT_DEFER_MAX", 128)), self.nbuf)
        assert self.nbuf < int(env.get("VKSIFT_DEFER_CHUNK", 16)), "the model leaves the early launch of idle GPUs out"
        self.defer = not env.get("VKSIFT_DEFER", "1").startswith("0") and self.nbuf >= 2 and self.defer_max >= 2
        self.pend, self.pend_first, self.pend_shape = 0, 0, None
        self.epoch, self.batch_mode, self.defer_grow = 0, False, False
        self.prof, self.matched, self.described = False, False, False
        self.entries = []                # [key, exec, stamp]
        self.stamp, self.miss_run, self.next_exec = 0, 0, 0
        self.events = []                 # of the current call
        self.launches = []               # (call index, count, eligible): every detection launched, in order

    # -------------------------------------------------------------------------------- the cache
    def drop_all(self):
        if self.entries:
            self.events.append(("drop", sorted(e[1] for e in self.entries)))
        self.entries = []

    def launch(self, w, h, first, count, src):
        """one detection reaches the GPU. src: "host" or the device block"""
        octave = has_octave(w, h, self.ups)
        obs = self.obs() if octave else {"post": False, "grew": False}    # (observed at the extraction launch: an image without an octave has none)
        if obs["grew"]:
            self.drop_all()
        overlap = self.pingpong and octave and count >= self.overlap_min
        if src == "host":
            src = "h_input" if count == 1 and w * h <= 1 << 20 else "d_input"
        dense = self.matched and octave
        eligible = self.use_graphs and not self.prof and not overlap and not (self.pingpong and self.pyr_nbuf == 2) and count * w * h <= self.graph_max_pixels
        self.launches.append((self.call, count, eligible))
        if not eligible:
            return
        key = (w, h, count, first, src, obs["post"], dense)
        for e in self.entries:
            if e[0] == key:
                self.stamp += 1
                e[2] = self.stamp
                self.miss_run = 0
                self.events.append(("replay", e[1]))
                return
        evicted = None
        if len(self.entries) == GRAPH_CACHE:
            victim = min(self.entries, key=lambda e: e[2])
            self.entries.remove(victim)
            evicted = victim[1]
        self.miss_run += 1
        if self.miss_run > GIVE_UP_AFTER:
            self.use_graphs = False      # for good; the entry it emptied stays empty
            self.events.append(("evict", evicted))
            return
        self.stamp += 1
        self.entries.append([key, self.next_exec, self.stamp])
        self.events.append(("capture", self.next_exec, evicted))
        self.next_exec += 1

    # -------------------------------------------------------------------------------- deferred submission
    def resize(self, cap):
        self.drop_all()
        self.det_cap = cap
        if not self.overlap_forced and self.bc < 8 and self.det_cap >= 8 and not self.pingpong:
            self.pingpong, self.overlap_min = True, 8

    def flush(self):
        if self.pend:
            n, self.pend = self.pend, 0
            self.launch(self.pend_shape[0], self.pend_shape[1], self.pend_first, n, "host")

    def sync(self):
        self.flush()
        if self.epoch:
            self.batch_mode, self.epoch = self.epoch >= 2, 0

    def detect(self, w, h, b):
        run = self.epoch > 0 or self.batch_mode
        self.epoch += 1
        if self.defer and (run or self.pend) and not self.prof:
            if self.pend and (b != self.pend_first + self.pend or (w, h) != self.pend_shape):
                self.flush()
            elif not self.pend and self.defer_grow and self.det_cap < self.defer_max:
                self.defer_grow = False
                self.resize(min(2 * self.det_cap, self.defer_max))
            if self.det_cap < 2:
                self.resize(2)
            if self.pend == 0:
                self.pend_first, self.pend_shape = b, (w, h)
            self.pend += 1
            if self.pend >= min(self.det_cap, self.defer_max):
                self.defer_grow = self.det_cap < self.defer_max
                self.flush()
            return
        self.flush()
        self.launch(w, h, b, 1, "host")

    # -------------------------------------------------------------------------------- the walk
    def obs(self):
        return self.observed.pop(0) if self.observed else {"post": False, "grew": False}

    def step(self, call, op, observed):
        """the cache events of one call; observed: the observations of the detections it launches, in order"""
        self.call, self.events, self.observed = call, [], list(observed)
        name = op[0]
        if name == "detect":
            self.detect(op[1], op[2], op[3])
        elif name in ("batch", "batchdev"):
            self.sync()
            self.launch(op[1], op[2], op[3], op[4], "host" if name == "batch" else ("dev", op[5]))
        elif name == "prof":
            self.sync()
            self.prof = bool(op[1])
        elif name == "match":
            self.sync()
            self.matched = True
        elif name == "describe":
            self.sync()
            if not self.described:       # the first describe call extends the descriptor scale table, an argument of every captured descriptor launch
                self.described = True
                self.drop_all()
        elif name in ("num", "download", "avail"):
            self.sync()
        return self.events
