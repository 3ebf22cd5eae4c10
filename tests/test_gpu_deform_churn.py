"""A churn of the deformation stores (st_deform.cpp): skins, morph targets, poses, weights, mesh and instance replacement and the
deformation-motion switch interleaved over the shared free lists of the posed, bind and target stores.

A fixed-seed sequence of STEPS steps, one operation and one tick each. After every tick st_debug_read_posed of every instance is compared
bit for bit with tests/skin_ref.py and tests/morph_ref.py applied to that instance's current palette and weights (an instance without a
deformation must answer with today's error): a region handed out twice, or one that kept stale contents, shows as one instance's bits.

What the sequence must contain is derived from st_debug_skinning, st_debug_morphing and st_debug_deformation between the steps (Events below)
and asserted, so that a sequence that never grows a store or never reuses a range cannot pass:
  posed_growth              a tick computed more triangles than the instances this step touched can account for: only a posed store that was
                            reallocated computes every region again
  posed_growth_previous     ... while the tick left some instance a previous region (st_debug_deformation)
  posed_reuse               since the last (possible) growth the ticks handed out more posed triangles than half of everything handed out up
                            to that growth — 1.5 x the store's size then is its allocation — and the store did not grow: a freed range was reused
  bind_reuse_by_morph_only  a mesh with targets and no skin was first computed (the morph counter moved) when a skin whose instances a tick
                            had computed, of at least its size, had been dropped and no later placement can have used its range up:
                            first fit reuses it
  target_growth             the device holds more target units (st_debug_morphing bytes / 72) than 1.5 x everything placed up to the store's
                            last known reallocation: it was reallocated again with other sets resident
"""
import functools

import numpy as np
import pytest

import morph_ref
import test_gpu_deform_motion as dm
from skin_ref import bind_store, skin
from strolle_amd import Buffer, CameraMode, Engine, Instance, Material, Mesh, StrolleError, scenes

pytestmark = pytest.mark.gpu

REBUILD, AUTO = 0, 4
SEED, STEPS = 14, 40
SIZES = (5, 64, 130, 257)            # both sides of one and two kSkinBlock (128) paddings
MESH, INST, MAT = 9000, 9100, 9000
SIZE = (64, 48)
NO_DEFORMATION = "neither a pose nor morph weights"
EXPECTED = {}
EVENTS = ("posed_growth", "posed_growth_previous", "posed_reuse", "bind_reuse_by_morph_only", "target_growth")


def xform(i):
    return np.array([[0.15, 0, 0, -0.6 + 0.4 * (i % 4)], [0, 0.15, 0, 0.4 + 0.6 * (i // 4)], [0, 0, 0.15, 0.0]], np.float32)


def random_mesh(rng, n):
    pos = rng.uniform(-1, 1, (n, 3, 3)).astype(np.float32)
    nrm = rng.normal(size=(n, 3, 3)); nrm /= np.linalg.norm(nrm, axis=2, keepdims=True)
    return Mesh(pos, nrm.astype(np.float32), rng.uniform(0, 1, (n, 3, 2)).astype(np.float32))


class Churn:
    """The engine under test, what each mesh and instance holds (the model the references are computed from), and the event bookkeeping."""

    def __init__(self, exact, mode):
        self.rng = np.random.default_rng(SEED)
        self.e = Engine(device=0, exact=exact)
        scenes.build_cornell(self.e); self.e.set_seed(3); self.e.set_bvh_refresh(mode); self.e.keep_all_planes(True)
        self.e.insert_material(MAT, Material(base_color=(0.2, 0.7, 0.3, 1.0)))
        self.meshes, self.insts, self.motion, self.ticks = {}, {}, False, 0
        self.events = dict.fromkeys(EVENTS, False)
        self.touched = set()
        self.posed_taken = self.posed_base = self.posed_since = 0     # triangles handed out: ever, up to the last (possible) growth, since
        self.freed_binds = []                                         # triangle counts of bind ranges that computed skins gave back
        self.bind_placed = {}                                         # mesh -> "skin" | "morph": whose bind range the counters saw computed
        self.units_placed = 0; self.units_cap = None                  # target units placed ever; 3 x that (half units) at the last known reallocation
        for k, n in enumerate(SIZES):
            self.new_mesh(MESH + k, n)
            for j in range(2):
                i = INST + 2 * k + j
                self.insts[i] = dict(mesh=MESH + k, pose=None, weights=None, region=False, slot=2 * k + j)
                self.e.insert_instance(i, Instance(MESH + k, MAT, xform(2 * k + j)))
        self.e.tick()

    # ---- the model
    def new_mesh(self, h, n):
        mesh = random_mesh(self.rng, n)
        self.e.insert_mesh(h, mesh)
        self.give_bind(h)
        self.meshes[h] = dict(n=n, bind=bind_store(mesh), skin=None, targets=None)
        for i, s in self.insts.items():
            if s["mesh"] == h:
                s.update(pose=None, weights=None, region=False)

    def give_bind(self, h):
        if self.bind_placed.pop(h, None) == "skin":
            self.freed_binds.append(self.meshes[h]["n"])

    def of_mesh(self, h):
        return [i for i, s in self.insts.items() if s["mesh"] == h]

    def deformed(self, s):
        return s["pose"] is not None or s["weights"] is not None

    def touch(self, i):
        s = self.insts[i]
        if not self.deformed(s):
            s["region"] = False
        self.touched.add(i)

    def expected(self, i):
        """Computed by the first run, shared by the others: the sequence is the same in all of them."""
        key = (self.ticks, i)
        if key not in EXPECTED:
            s = self.insts[i]; m = self.meshes[s["mesh"]]
            out = m["bind"] if s["weights"] is None else morph_ref.morph(m["bind"], *m["targets"], s["weights"])
            EXPECTED[key] = out if s["pose"] is None else skin(out, m["skin"][0], m["skin"][1], s["pose"])
        return EXPECTED[key]

    # ---- the operations
    def op_set_skin(self):
        h = MESH + int(self.rng.integers(len(SIZES))); m = self.meshes[h]
        joints = int(self.rng.integers(1, 9))
        jt = self.rng.integers(0, joints, (3 * m["n"], 4)); wt = self.rng.uniform(0.05, 1.0, (3 * m["n"], 4)).astype(np.float32)
        wt[self.rng.random(wt.shape) < 0.2] = 0.0; wt[:, 0] = np.maximum(wt[:, 0], np.float32(0.1))
        self.e.set_skin(h, jt, wt, joints)
        if self.bind_placed.get(h) == "skin":
            self.give_bind(h)
        m["skin"] = (jt, wt, joints)
        for i in self.of_mesh(h):
            if self.insts[i]["pose"] is not None or self.motion:   # (with the switch on a region computed from an earlier pose is forgotten too)
                self.insts[i]["pose"] = None; self.touch(i)

    def op_set_targets(self):
        h = MESH + int(self.rng.integers(len(SIZES))); m = self.meshes[h]
        k = int(self.rng.integers(1, 5))
        dp = self.rng.uniform(-0.3, 0.3, (k, m["n"], 3, 3)).astype(np.float32); dn = self.rng.uniform(-0.5, 0.5, (k, m["n"], 3, 3)).astype(np.float32)
        self.e.set_morph_targets(h, dp, dn)
        if self.bind_placed.get(h) == "morph":
            self.bind_placed.pop(h)
        m["targets"] = (dp, dn)
        for i in self.of_mesh(h):
            if self.insts[i]["weights"] is not None or self.motion:
                self.insts[i]["weights"] = None; self.touch(i)

    def pick_instance(self, what):
        good = [i for i, s in self.insts.items() if self.meshes[s["mesh"]][what] is not None]
        pool = good if good and self.rng.random() < 0.85 else list(self.insts)
        return pool[int(self.rng.integers(len(pool)))]

    def op_set_pose(self):
        i = self.pick_instance("skin"); s = self.insts[i]; sk = self.meshes[s["mesh"]]["skin"]
        if sk is None:
            with pytest.raises(StrolleError, match="has no skin"):
                self.e.set_pose(i, np.zeros((1, 3, 4), np.float32))
            return
        if s["pose"] is not None and self.rng.random() < 0.2:
            self.e.set_pose(i, None); s["pose"] = None
        else:
            pose = np.tile(np.eye(3, 4, dtype=np.float32), (sk[2], 1, 1)) + self.rng.uniform(-0.3, 0.3, (sk[2], 3, 4)).astype(np.float32)
            self.e.set_pose(i, pose); s["pose"] = pose
        self.touch(i)

    def op_set_weights(self):
        i = self.pick_instance("targets"); s = self.insts[i]; tg = self.meshes[s["mesh"]]["targets"]
        if tg is None:
            with pytest.raises(StrolleError, match="has no morph targets"):
                self.e.set_morph_weights(i, np.ones(1, np.float32))
            return
        k, r = len(tg[0]), self.rng.random()
        if s["weights"] is not None and r < 0.2:
            w = None if r < 0.1 else np.zeros(k, np.float32)         # cleared, or all zero: the same thing
            self.e.set_morph_weights(i, w); s["weights"] = None
        else:
            w = self.rng.uniform(-1.0, 2.0, k).astype(np.float32)
            if k > 1:
                w[int(self.rng.integers(k))] = 0.0
            self.e.set_morph_weights(i, w); s["weights"] = w
        self.touch(i)

    def op_reinsert_mesh(self):
        h = MESH + int(self.rng.integers(len(SIZES)))
        for i in self.of_mesh(h):
            self.touched.add(i)
        self.new_mesh(h, int(self.rng.choice([n for n in SIZES if n != self.meshes[h]["n"]])))
        for i in self.of_mesh(h):
            self.e.insert_instance(i, Instance(h, MAT, xform(self.insts[i]["slot"])))   # (its triangle slots are for the old count)

    def op_reinsert_instance(self):
        i = INST + int(self.rng.integers(len(self.insts))); s = self.insts[i]
        self.e.remove_instance(i)
        s.update(pose=None, weights=None, region=False)
        self.tick_and_check()
        s["mesh"] = MESH + int(self.rng.integers(len(SIZES)))
        self.e.insert_instance(i, Instance(s["mesh"], MAT, xform(s["slot"])))
        self.touched.add(i)

    def op_toggle_motion(self):
        self.motion = not self.motion
        self.e.set_deformation_motion(self.motion)

    OPS = (("op_set_skin", 0.12), ("op_set_targets", 0.12), ("op_set_pose", 0.25), ("op_set_weights", 0.25), ("op_reinsert_mesh", 0.08),
           ("op_reinsert_instance", 0.10), ("op_toggle_motion", 0.08))

    # ---- a tick, the per-step assertion and the events
    def counters(self):
        sk, mo, de = self.e.skinning_stats(), self.e.morphing_stats(), self.e.deformation_stats()
        return dict(skinned=sk[1], morphed=mo[1], units=mo[2] // 72, with_previous=de[0], previous=de[1] // 96)

    def tick_and_check(self):
        before = self.counters()
        self.e.tick(); self.ticks += 1
        after = self.counters()
        deformed = [i for i, s in self.insts.items() if self.deformed(s)]
        for i, s in self.insts.items():
            if i in deformed:
                got, want = self.e.read_posed(i), self.expected(i)
                assert got.tobytes() == want.tobytes(), f"instance {i}: {np.count_nonzero(np.any(got.view(np.uint32) != want.view(np.uint32), axis=1))} of {len(want)} posed triangles differ"
            else:
                with pytest.raises(StrolleError, match=NO_DEFORMATION):
                    self.e.read_posed(i)
        n_of = lambda i: self.meshes[self.insts[i]["mesh"]]["n"]
        jobs = lambda i: n_of(i) * ((self.insts[i]["pose"] is not None) + (self.insts[i]["weights"] is not None))
        computed = (after["skinned"] - before["skinned"]) + (after["morphed"] - before["morphed"])
        touched = [i for i in deformed if i in self.touched]
        # posed store: what this tick handed out, and whether it (may have) reallocated
        taken = sum(n_of(i) for i in deformed if not self.insts[i]["region"]) + max(0, after["previous"] - before["previous"])
        grew = computed > sum(jobs(i) for i in touched)               # without a reallocation only touched instances are computed
        maybe_grew = grew or (taken and len(touched) == len(deformed))   # (every region was computed anyway: a growth would not show)
        self.posed_taken += taken; self.posed_since += taken
        if maybe_grew:
            self.posed_base, self.posed_since = self.posed_taken, 0
        elif taken and 2 * self.posed_since > self.posed_base:
            self.events["posed_reuse"] = True
        self.events["posed_growth"] |= grew
        self.events["posed_growth_previous"] |= grew and after["with_previous"] > 0
        # bind store: a bind range is placed by the first tick that computes an instance of the mesh
        for i in touched:
            h = self.insts[i]["mesh"]; m = self.meshes[h]
            kind = "morph" if m["skin"] is None else "skin"          # (a mesh with a skin places the skin's range, whatever the instance holds)
            if self.bind_placed.get(h) == kind:
                continue
            fits = [n for n in self.freed_binds if n >= m["n"]]
            if fits:
                self.freed_binds.remove(max(fits))                    # (whichever range first fit took: never overstate what is left)
            if kind == "morph":
                assert after["morphed"] > before["morphed"], "a mesh without a skin is computed by the morph stage"
                self.events["bind_reuse_by_morph_only"] |= bool(fits)
            self.bind_placed[h] = kind
        # target store
        self.units_placed += max(0, after["units"] - before["units"])
        if after["units"] > before["units"] and (self.units_cap is None or 2 * after["units"] > self.units_cap):
            self.events["target_growth"] |= self.units_cap is not None and before["units"] > 0
            self.units_cap = 3 * self.units_placed                    # (in half units: 1.5 x)
        for i in deformed:
            self.insts[i]["region"] = True
        self.touched.clear()

    def run(self):
        names, p = [n for n, _ in self.OPS], np.array([w for _, w in self.OPS])
        try:
            for step in range(STEPS):
                getattr(self, names[int(self.rng.choice(len(names), p=p / p.sum()))])()
                self.tick_and_check()
            # one frame at the end, with the switch on and every deformed instance deformed again: its velocity plane
            self.e.set_deformation_motion(True)
            for _ in range(2):
                for i, s in self.insts.items():
                    if s["pose"] is not None:
                        s["pose"] = s["pose"] * np.float32(1.05); self.e.set_pose(i, s["pose"]); self.touched.add(i)
                    if s["weights"] is not None:
                        s["weights"] = s["weights"] * np.float32(1.05); self.e.set_morph_weights(i, s["weights"]); self.touched.add(i)
                self.motion = True
                self.tick_and_check()
            cam = self.e.create_camera(scenes.cornell_camera(SIZE, CameraMode.IMAGE))
            planes = dm.frame_planes(self.e, cam, dm.new_out(SIZE))
            return dict(self.events), planes[Buffer.VELOCITY_MAP]
        finally:
            self.e.close()


@functools.lru_cache(maxsize=None)
def churned(exact, mode):
    return Churn(exact, mode).run()


@pytest.mark.parametrize("mode", [AUTO, REBUILD], ids=["auto", "rebuild"])
@pytest.mark.parametrize("exact", [True, False], ids=["exact", "fast"])
def test_churn_keeps_every_instances_bits(exact, mode):
    events, _ = churned(exact, mode)
    assert all(events.values()), f"the sequence lacks {[k for k, v in events.items() if not v]}: choose another SEED"


def test_velocity_plane_is_the_same_under_auto_and_rebuild():
    (_, auto), (_, rebuild) = churned(True, AUTO), churned(True, REBUILD)
    assert auto.tobytes() == rebuild.tobytes()
    assert np.any(auto != 0.0), "nothing moved in the last frame"
