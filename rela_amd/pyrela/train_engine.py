"""Ape-X training on the device-resident path: actor shard, env, replay and learner on one GPU, no per-step host traffic.

    python -m rela_amd.pyrela.train_engine            # Catch (csrc/catch_game.h), the one env here with something to learn

Where main.py drives the threaded `rela` module with host envs, this loop drives the objects behind the benchmark:

    FFReplay  <-  ApexActorEngine  <->  DeviceCatchEnv           (actor stream)
       |-> sample -> HipApexLearner.step -> update_priority      (learner stream)
       '------------- learner.publish -> the actors' FFNetHandles, every --actor_sync_freq updates

One tick = act, env.step, post_step(reward, terminal on the device), env.render into the slot post_step released
(rela_amd/device_env.py says why the step and the frame are two launches for a shard with a replay).  Once the replay
holds --burn_in_frames transitions a tick is followed by --updates_per_tick learner updates.  After every epoch of
--epoch_len updates a second, replay-less engine plays --eval_rows games greedily (eps 0, a fixed seed, exactly
--episode_len ticks, fused step-and-render launches) with the current online weights: its mean return is the score.
Flags shared with main.py keep its names and defaults; the update-rule flags go through main.UpdateRules.
"""
import argparse
import math
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from rela_amd.pyrela import main as _main  # noqa: E402
from rela_amd.pyrela import utils  # noqa: E402

NUM_ACTION = 18
HISTORY_KEYS = ("epoch", "updates", "ticks", "num_act", "seconds", "env_steps_per_s", "grad_steps_per_s", "loss",
                "train_return", "train_return_low_eps", "train_episodes", "eval_return", "replay_size", "lr",
                "weights_moved", "actor_net_version")


def parse_args(argv=None):
    p = argparse.ArgumentParser(description="Ape-X on the device-resident actor engine and the device Catch env (MI355X)")
    p.add_argument("--algo", type=str, default="apex", help="apex only: the R2D2 engine loop is not built")
    p.add_argument("--game", type=str, default="catch", help="catch only")
    p.add_argument("--seed", type=int, default=10002)
    p.add_argument("--device", type=str, default="cuda:0")
    # as main.py
    p.add_argument("--multi_step", type=int, default=3)
    p.add_argument("--gamma", type=float, default=0.997)
    p.add_argument("--lr", type=float, default=6.25e-5)
    p.add_argument("--eps", type=float, default=1.5e-4)
    p.add_argument("--grad_clip", type=float, default=40)
    p.add_argument("--batchsize", type=int, default=512)
    p.add_argument("--priority_exponent", type=float, default=0.6)
    p.add_argument("--importance_exponent", type=float, default=0.4)
    p.add_argument("--act_base_eps", type=float, default=0.4)
    p.add_argument("--act_eps_alpha", type=float, default=7)
    p.add_argument("--actor_sync_freq", type=int, default=20)
    p.add_argument("--episode_len", type=int, default=200)
    p.add_argument("--value_rescale", type=float, default=0.0)
    p.add_argument("--num_update_between_sync", type=int, default=500,
                   help="target net copy every so many updates (main.py: 2500; this loop's default run is 20,000 updates)")
    p.add_argument("--learner_precision", type=str, default="f32", choices=_main.LEARNER_PRECISIONS)
    p.add_argument("--rmsprop_alpha", type=float, default=0.99)
    p.add_argument("--rmsprop_centered", type=int, default=0)
    p.add_argument("--adam_beta1", type=float, default=0.9)
    p.add_argument("--adam_beta2", type=float, default=0.999)
    p.add_argument("--lr_warmup_updates", type=int, default=0)
    p.add_argument("--lr_final", type=float, default=None)
    p.add_argument("--lr_decay_updates", type=int, default=0)
    p.add_argument("--target_tau", type=float, default=0.0)
    p.add_argument("--target_update_freq", type=int, default=1)
    # this loop's own; the sizes are those of a run of a few minutes on one GPU, not main.py's
    p.add_argument("--rows", type=int, default=1024, help="envs = rows of the actor shard")
    p.add_argument("--group_rows", type=int, default=64, help="rows per group: the envs of one reference actor thread")
    p.add_argument("--eval_rows", type=int, default=256, help="games of the greedy evaluation after every epoch; 0 = none")
    p.add_argument("--updates_per_tick", type=int, default=1, help="learner updates after every tick once the replay is warm")
    p.add_argument("--act_precision", type=str, default="f32", choices=("f32", "bf16x2", "f32x3"),
                   help="arithmetic of the actors' forwards (FFNetHandle.set_precision)")
    p.add_argument("--dedup", type=str, default="none", choices=("none", "stack", "plane"),
                   help="frame-stack de-duplication of the replay; Catch's stack slides, so plane is valid")
    p.add_argument("--replay_buffer_size", type=int, default=1 << 18)
    p.add_argument("--burn_in_frames", type=int, default=20000)
    p.add_argument("--num_epoch", type=int, default=20)
    p.add_argument("--epoch_len", type=int, default=1000)
    args = p.parse_args(argv)
    if args.algo != "apex":
        p.error("--algo %s: this loop is Ape-X only (the R2D2 actor shard is wired and tested, its engine loop is not "
                "built); rela_amd/pyrela/main.py --algo r2d2 --game catch trains R2D2 on the threaded path" % args.algo)
    if args.game != "catch":
        p.error("--game %s: the only device-resident env is catch" % args.game)
    if args.rows < 1 or args.group_rows < 1 or args.rows % args.group_rows:
        p.error("--rows must be a positive multiple of --group_rows")
    if args.updates_per_tick < 1 or args.epoch_len < 1 or args.num_epoch < 1 or args.eval_rows < 0:
        p.error("--updates_per_tick, --epoch_len and --num_epoch must be >= 1, --eval_rows >= 0")
    if args.burn_in_frames > args.replay_buffer_size or args.batchsize > args.replay_buffer_size:
        p.error("--burn_in_frames and --batchsize cannot exceed --replay_buffer_size")
    if 4 * args.rows > args.replay_buffer_size:
        # the ring has 1.25 x capacity slots and a sample evicts down to the capacity: a tick's block must fit in between
        p.error("--replay_buffer_size must be at least 4 x --rows")
    return args


def evaluate(eval_engine, online, args, seed):
    """Greedy games on the device: `eval_engine` (replay=None, eps 0) plays its rows on a fresh DeviceCatchEnv seeded
    `seed` for exactly episode_len ticks, one episode per row.  -> (mean return, per-row returns as an int32 cuda tensor)"""
    from rela_amd.device_env import DeviceCatchEnv

    env = DeviceCatchEnv(eval_engine.R, eval_engine.A, args.episode_len, seed, str(eval_engine.device))
    env.reset(eval_engine.next_obs_slot())
    for _ in range(args.episode_len):
        action = eval_engine.act(online)
        env.step(action, eval_engine.next_obs_slot())
    st = env.episode_stats()
    env.close()
    assert st["episodes"] == eval_engine.R, "every row finishes exactly one episode in episode_len ticks"
    returns = st["rows"]["last_return"]
    return float(returns.double().mean()), returns


def train(args, on_epoch=None):
    """-> history: one dict per epoch with the keys HISTORY_KEYS; on_epoch(record) is called after every epoch."""
    from rela_amd import _capi as capi
    from rela_amd.device_env import DeviceCatchEnv
    from rela_amd.engine import ApexActorEngine, FFNetHandle
    from rela_amd.learner import HipApexLearner
    from rela_amd.pyrela.apex import ApexAgent
    from rela_amd.pyrela.net import AtariFFNet
    from rela_amd.replay import FFReplay

    if not torch.cuda.is_available():
        raise SystemExit("train_engine needs an MI355X: no HIP device visible and there is no CPU path")
    precision = _main.learner_precision(args)
    rules = _main.UpdateRules(args)
    device = args.device
    torch.cuda.set_device(torch.device(device))
    torch.manual_seed(args.seed + 2)
    A, R = NUM_ACTION, args.rows

    agent = ApexAgent(lambda: AtariFFNet(A), args.multi_step, args.gamma, args.value_rescale).to(device)
    learner = HipApexLearner.from_agent(agent, args.batchsize, lr=args.lr, eps=args.eps, grad_clip=args.grad_clip,
                                        **rules.learner_kw())
    if precision != "f32":
        learner.set_precision(precision)
    online, target = FFNetHandle(A, device), FFNetHandle(A, device)
    online.load_state_dict(agent.online_net.state_dict())
    target.load_state_dict(agent.target_net.state_dict())
    online.set_precision(args.act_precision)
    target.set_precision(args.act_precision)
    initial = learner.flat()[0].clone()

    dedup = None if args.dedup == "none" else args.dedup
    replay = FFReplay(args.replay_buffer_size, args.seed, args.priority_exponent, args.importance_exponent, 0, A, device,
                      dedup=dedup, guard_units=(args.multi_step + 8) * R)
    eps = utils.generate_eps(args.act_base_eps, args.act_eps_alpha, R)
    engine = ApexActorEngine(R, args.group_rows, A, args.multi_step, args.gamma, replay, eps, device, seed=args.seed)
    if args.value_rescale > 0:
        engine.set_value_rescale(args.value_rescale)
    env = DeviceCatchEnv(R, A, args.episode_len, args.seed, device)
    low_eps = torch.as_tensor(sorted(range(R), key=lambda i: eps[i])[:max(R // 4, 1)], device=device)
    eval_engine = None
    if args.eval_rows > 0:
        eval_engine = ApexActorEngine(args.eval_rows, args.eval_rows, A, args.multi_step, args.gamma, None,
                                      [0.0] * args.eval_rows, device, seed=args.seed + 1)

    actor_stream = torch.cuda.Stream(device=device)
    learner_stream = torch.cuda.Stream(device=device)
    actor_stream.wait_stream(torch.cuda.current_stream(device))
    learner_stream.wait_stream(torch.cuda.current_stream(device))
    ticks = 0

    def tick():
        with torch.cuda.stream(actor_stream):
            action = engine.act(online)
            reward, terminal = env.step(action)
            # (non-blocking: a full ring drops the block instead of waiting for a sample this thread would have to issue)
            engine.post_step(reward, terminal, online, target, nonblocking=True)
            env.render(engine.next_obs_slot())

    def publish():
        learner_stream.wait_stream(actor_stream)
        learner.publish(online, target)
        actor_stream.wait_stream(learner_stream)

    with torch.cuda.stream(actor_stream):
        env.reset(engine.next_obs_slot())
    while replay.size() < max(args.burn_in_frames, args.batchsize):
        tick()
        ticks += 1
        if ticks % 64 == 0:
            actor_stream.synchronize()  # (bounds the launch queue)
    print("replay warm: %d transitions after %d ticks of %d rows" % (replay.size(), ticks, R), flush=True)

    history = []
    num_update = 0
    loss_sum = torch.zeros((), device=device)
    for epoch in range(args.num_epoch):
        torch.cuda.synchronize()
        t0 = time.time()
        ticks0 = ticks
        episodes0 = env.stats_dev()[0].clone()
        loss_sum.zero_()
        done = 0
        while done < args.epoch_len:
            tick()
            ticks += 1
            with torch.cuda.stream(learner_stream):
                for _ in range(min(args.updates_per_tick, args.epoch_len - done)):
                    rules.before_update(num_update, learner, None, None)
                    if num_update % args.actor_sync_freq == 0:
                        publish()
                    batch, weight = replay.sample(args.batchsize)
                    loss, priority = learner.step(batch, weight)
                    replay.update_priority(priority)
                    loss_sum += loss[0]
                    num_update += 1
                    done += 1
            if ticks % 16 == 0:
                actor_stream.synchronize()  # (bounds the launch queue; the learner's stream is read below)
        torch.cuda.synchronize()
        dt = time.time() - t0
        st = env.stats_dev().clone()
        finished = st[0] > episodes0
        last = st[2].double()

        def mean_last(values, mask):  # mean last_return of the rows that finished an episode this epoch
            return float(values[mask].mean()) if bool(mask.any()) else float("nan")

        rec = dict(epoch=epoch, updates=num_update, ticks=ticks, num_act=engine.num_act, seconds=dt,
                   env_steps_per_s=(ticks - ticks0) * R / dt, grad_steps_per_s=args.epoch_len / dt,
                   loss=float(loss_sum) / args.epoch_len, train_return=mean_last(last, finished),
                   train_return_low_eps=mean_last(last[low_eps], finished[low_eps]),
                   train_episodes=int((st[0] - episodes0).sum()), eval_return=float("nan"), replay_size=replay.size(),
                   lr=rules.lr_now, weights_moved=float((learner.flat()[0] - initial).norm()),
                   actor_net_version=int(capi.lib.rela_ffnet_version(online.h)))
        if eval_engine is not None:
            with torch.cuda.stream(learner_stream):
                publish()  # the current online weights
            with torch.cuda.stream(actor_stream):
                rec["eval_return"], _ = evaluate(eval_engine, online, args, args.seed + 1000003)
        if not math.isfinite(rec["loss"]):
            raise RuntimeError("epoch %d: the mean loss is %r" % (epoch, rec["loss"]))
        history.append(rec)
        print("epoch %d: %d updates, %.1fs, %.0f env-steps/s, %.1f grad-steps/s, loss %.5f, train return %.2f "
              "(lowest-eps quarter %.2f, %d episodes), eval return %.2f" % (
                  epoch, num_update, dt, rec["env_steps_per_s"], rec["grad_steps_per_s"], rec["loss"], rec["train_return"],
                  rec["train_return_low_eps"], rec["train_episodes"], rec["eval_return"]), flush=True)
        if on_epoch is not None:
            on_epoch(rec)
    torch.cuda.synchronize()
    for obj in (env, engine, eval_engine, replay, learner, online, target):
        if obj is not None:
            obj.close()
    return history


if __name__ == "__main__":
    train(parse_args())
