// Host-runtime stress program for sanitizer builds (ThreadSanitizer / AddressSanitizer):
// the threaded actor system, the TCP cluster layer and the full master/worker protocol,
// with fault injection, exactly as the CLIs run them - but in one process without Python,
// so the sanitizer sees every thread. Exit 0 = all rounds exact and clean shutdown.
//
//   build + run: python tools/sanitize.py --sanitize thread
#include <arpa/inet.h>
#include <netinet/in.h>
#include <sys/socket.h>
#include <unistd.h>

#include <atomic>
#include <map>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../cluster/cluster_node.h"
#include "../core/log.h"
#include "../runtime/allreduce_actors.h"
#include "../runtime/akka_endpoint.h"
#include "../runtime/control_bridge.h"
#include "../runtime/fault_injector.h"
#include "../runtime/launch_geometry.h"
#include "../runtime/loopback_plane.h"
#include "../runtime/plane_rounds.h"
#include "../runtime/plane_worker.h"
#include "../runtime/sdma_schedule.h"

using namespace mxar;

static bool wait_until(const std::function<bool()>& pred, double timeout_s) {
  const auto t0 = std::chrono::steady_clock::now();
  while (std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() < timeout_s) {
    if (pred()) return true;
    std::this_thread::sleep_for(std::chrono::milliseconds(5));
  }
  return false;
}

// In-process threaded cluster with reordering faults; exact thresholds.
static int run_local(int P, int N, int C, int rounds) {
  auto sys = std::make_shared<ActorSystem>("ClusterSystem", ActorSystem::Mode::Threaded, 4);
  std::atomic<bool> done{false};
  MasterParams mp{P, 1.f, 1.f, 1.f, 3, N, rounds - 1, C, false};
  ActorRef master = sys->actor_of(std::make_unique<MasterActor>(mp, [&](int) { done = true; }), "master");
  std::mutex mu;
  std::vector<std::vector<std::vector<float>>> outs(P);
  std::vector<ActorRef> refs;
  for (int k = 0; k < P; ++k) {
    DataSource src = [N, k](const AllReduceInputRequest& r) {
      std::vector<float> v(N);
      for (int i = 0; i < N; ++i) v[i] = static_cast<float>((i + r.iteration) * (k + 1));
      return AllReduceInput{make_host_payload(std::move(v))};
    };
    DataSink sink = [&, k](const AllReduceOutput& o) {
      std::lock_guard<std::mutex> g(mu);
      if (static_cast<int>(outs[k].size()) <= o.iteration) outs[k].resize(o.iteration + 1);
      outs[k][o.iteration] = o.data->to_host();
    };
    ActorRef w = sys->actor_of(std::make_unique<WorkerActor>(src, sink), "worker" + std::to_string(k));
    FaultPolicy fp;
    fp.delay_ms = 2;
    fp.delay_prob = 0.3;
    fp.kinds = {"ScatterBlock", "ReduceBlock"};
    fp.seed = 11 + k;
    refs.push_back(std::make_shared<FaultyRef>(sys.get(), w, fp));
  }
  for (auto& r : refs) master->tell(MemberUp{r, "worker", ""}, nullptr);
  const bool ok = wait_until([&] { return done.load(); }, 60);
  sys->await_idle(std::chrono::milliseconds(5000));
  sys->shutdown();
  if (!ok) {
    std::fprintf(stderr, "local cluster did not finish\n");
    return 1;
  }
  const float tri = P * (P + 1) / 2.f;
  for (int k = 0; k < P; ++k)
    for (int r = 0; r < rounds; ++r)
      for (int i = 0; i < N; ++i)
        if (std::fabs(outs[k][r][i] - (i + r) * tri) > 1e-3f) {
          std::fprintf(stderr, "bad sum worker %d round %d idx %d\n", k, r, i);
          return 1;
        }
  return 0;
}

// The control bridge (csrc/runtime/control_bridge.h): an external driver thread runs every
// round through a socket, pipelined (one StartAllreduce queued behind the round in flight),
// while churn threads connect, half-send and vanish - bridge reader / acceptor / reaper
// threads, the master's publishes and client fds all under the sanitizer.
static int connect_to(int port) {
  int fd = ::socket(AF_INET, SOCK_STREAM | SOCK_CLOEXEC, 0);
  sockaddr_in a{};
  a.sin_family = AF_INET;
  a.sin_port = htons(static_cast<uint16_t>(port));
  ::inet_pton(AF_INET, "127.0.0.1", &a.sin_addr);
  if (::connect(fd, reinterpret_cast<sockaddr*>(&a), sizeof(a)) != 0) {
    ::close(fd);
    return -1;
  }
  return fd;
}

static int run_bridge(int P, int N, int C, int rounds) {
  auto sys = std::make_shared<ActorSystem>("ClusterSystem", ActorSystem::Mode::Threaded, 4);
  std::atomic<bool> done{false};
  MasterParams mp{P, 1.f, 1.f, 1.f, 1, N, rounds - 1, C, false};
  mp.externalRounds = true;
  auto actor = std::make_unique<MasterActor>(mp, [&](int) { done = true; });
  auto bridge = ControlBridge::start("127.0.0.1", 0);
  actor->set_bridge(bridge);
  ActorRef master = sys->actor_of(std::move(actor), "master");
  bridge->attach(master, master->path());
  const int port = bridge->port();
  std::atomic<int> sinks{0};
  for (int k = 0; k < P; ++k) {
    DataSource src = [N](const AllReduceInputRequest& r) {
      std::vector<float> v(N, static_cast<float>(r.iteration));
      return AllReduceInput{make_host_payload(std::move(v))};
    };
    DataSink sink = [&](const AllReduceOutput&) { sinks++; };
    ActorRef w = sys->actor_of(std::make_unique<WorkerActor>(src, sink), "worker" + std::to_string(k));
    master->tell(MemberUp{w, "worker", ""}, nullptr);
  }
  std::atomic<bool> stop_churn{false};
  std::vector<std::thread> churn;
  for (int t = 0; t < 3; ++t)
    churn.emplace_back([&, t] {
      for (int i = 0; !stop_churn.load(); ++i) {
        int fd = connect_to(port);
        if (fd < 0) continue;
        char b[32];
        (void)!::recv(fd, b, sizeof(b), 0);
        if ((i + t) % 2) (void)!::send(fd, "{\"type\":\"Sta", 12, MSG_NOSIGNAL);
        ::close(fd);
      }
    });
  int completed = 0;
  std::string err;
  {
    int fd = -1;
    for (int i = 0; i < 100 && fd < 0; ++i) fd = connect_to(port);
    std::string buf;
    auto line = [&]() -> std::map<std::string, std::string> {
      for (;;) {
        if (auto nl = buf.find('\n'); nl != std::string::npos) {
          std::string l = buf.substr(0, nl);
          buf.erase(0, nl + 1);
          std::map<std::string, std::string> kv;
          if (!parse_flat_json(l, kv)) kv["type"] = l.find("InitWorkers") != std::string::npos ? "InitWorkers" : "?";
          return kv;
        }
        char tmp[4096];
        ssize_t n = ::recv(fd, tmp, sizeof(tmp), 0);
        if (n <= 0) return {{"type", "EOF"}};
        buf.append(tmp, static_cast<size_t>(n));
      }
    };
    auto start = [&](int r) {
      std::string l = "{\"type\":\"StartAllreduce\",\"round\":" + std::to_string(r) + "}\n";
      (void)!::send(fd, l.data(), l.size(), MSG_NOSIGNAL);
    };
    std::map<std::string, std::string> m;
    do m = line(); while (m["type"] != "InitWorkers" && m["type"] != "EOF");
    int next = 0;
    start(next++);
    start(next++);
    while (completed < rounds) {
      m = line();
      if (m["type"] == "EOF" || m["type"] == "Error") {
        err = "bridge driver got " + m["type"] + " " + m["reason"];
        break;
      }
      if (m["type"] == "RoundComplete") ++completed;
      if (m["type"] == "Accepted" && std::stoi(m["round"]) == next - 1 && next < rounds) start(next++);
    }
    ::close(fd);
  }
  stop_churn = true;
  for (auto& t : churn) t.join();
  const bool ok = err.empty() && wait_until([&] { return done.load(); }, 30);
  sys->await_idle(std::chrono::milliseconds(5000));
  sys->shutdown();
  bridge.reset();
  if (!ok) {
    std::fprintf(stderr, "bridge-driven job failed: %s (rounds %d)\n", err.c_str(), completed);
    return 1;
  }
  if (sinks.load() != P * rounds) {
    std::fprintf(stderr, "bridge-driven job: %d outputs, want %d\n", sinks.load(), P * rounds);
    return 1;
  }
  return 0;
}

// Bridge teardown: (1) a client that connects and never reads while the master
// runs rounds on its own - its queue overflows and it is dropped, the rounds never stall on
// its socket; (2) the system shuts down while another client floods StartAllreduce, with
// the master holding the ONLY reference to the bridge, so the master (and the bridge's
// owner reference) can die inside a reader's tell().
static int run_bridge_teardown(int P, int N, int C, int rounds) {
  auto sys = std::make_shared<ActorSystem>("ClusterSystem", ActorSystem::Mode::Threaded, 4);
  std::atomic<bool> done{false};
  MasterParams mp{P, 1.f, 1.f, 1.f, 1, N, rounds - 1, C, false};
  auto actor = std::make_unique<MasterActor>(mp, [&](int) { done = true; });
  int port = 0;
  {
    auto bridge = ControlBridge::start("127.0.0.1", 0);
    bridge->set_max_queued_bytes(4096);
    actor->set_bridge(bridge);
    port = bridge->port();
    ActorRef master = sys->actor_of(std::move(actor), "master");
    bridge->attach(master, master->path());
    int lazy = connect_to(port);  // connects, never reads
    if (lazy >= 0) {
      int small = 4096;
      ::setsockopt(lazy, SOL_SOCKET, SO_RCVBUF, &small, sizeof(small));
    }
    std::this_thread::sleep_for(std::chrono::milliseconds(20));
    for (int k = 0; k < P; ++k) {
      DataSource src = [N](const AllReduceInputRequest& r) {
        std::vector<float> v(N, static_cast<float>(r.iteration));
        return AllReduceInput{make_host_payload(std::move(v))};
      };
      ActorRef w = sys->actor_of(std::make_unique<WorkerActor>(src, [](const AllReduceOutput&) {}),
                                 "worker" + std::to_string(k));
      master->tell(MemberUp{w, "worker", ""}, nullptr);
    }
    const bool ok = wait_until([&] { return done.load(); }, 60);
    if (lazy >= 0) ::close(lazy);
    if (!ok) {
      std::fprintf(stderr, "bridge teardown: rounds stalled behind a client that never reads\n");
      sys->shutdown();
      return 1;
    }
  }  // from here the master actor owns the only reference to the bridge
  std::atomic<bool> stop_flood{false};
  std::thread flood([&] {
    int fd = connect_to(port);
    if (fd < 0) return;
    const std::string l = "{\"type\":\"StartAllreduce\",\"round\":1}\n{\"type\":\"Status\"}\n";
    while (!stop_flood.load())
      if (::send(fd, l.data(), l.size(), MSG_NOSIGNAL) <= 0) break;
    ::close(fd);
  });
  std::this_thread::sleep_for(std::chrono::milliseconds(50));
  sys->shutdown();  // drops the master -> ~MasterActor stops the bridge mid-flood
  stop_flood = true;
  flood.join();
  return 0;
}

// The round engine on host memory: master + P PlaneWorkerActors over LoopbackRoundPlanes
// (plane completion threads, hub mutex, actor mailboxes all live under the sanitizer).
static int run_plane(int P, int N, int C, int rounds) {
  auto sys = std::make_shared<ActorSystem>("ClusterSystem", ActorSystem::Mode::Threaded, 4);
  std::atomic<bool> done{false};
  MasterParams mp{P, 1.f, 1.f, 1.f, 1, N, rounds - 1, C, false};
  ActorRef master = sys->actor_of(std::make_unique<MasterActor>(mp, [&](int) { done = true; }), "master");
  std::mutex mu;
  std::vector<std::vector<std::vector<float>>> outs(P);
  std::vector<std::shared_ptr<LoopbackRoundPlane>> planes;
  std::vector<ActorRef> refs;
  for (int k = 0; k < P; ++k) {
    DataSource src = [N, k](const AllReduceInputRequest& r) {
      std::vector<float> v(N);
      for (int i = 0; i < N; ++i) v[i] = static_cast<float>((i + r.iteration) * (k + 1));
      return AllReduceInput{make_host_payload(std::move(v))};
    };
    DataSink sink = [&, k](const AllReduceOutput& o) {
      std::lock_guard<std::mutex> g(mu);
      if (static_cast<int>(outs[k].size()) <= o.iteration) outs[k].resize(o.iteration + 1);
      outs[k][o.iteration] = o.data->to_host();
    };
    planes.push_back(make_loopback_plane("stress"));
    refs.push_back(sys->actor_of(std::make_unique<PlaneWorkerActor>(src, sink, planes.back()), "pw" + std::to_string(k)));
  }
  for (int k = 0; k < P; ++k) master->tell(MemberUp{refs[k], "worker", "", planes[k]->descriptor()}, nullptr);
  const bool ok = wait_until([&] { return done.load(); }, 60);
  for (auto& p : planes) p->drain();
  sys->await_idle(std::chrono::milliseconds(5000));
  sys->shutdown();
  if (!ok) {
    std::fprintf(stderr, "plane cluster did not finish\n");
    return 1;
  }
  const float tri = P * (P + 1) / 2.f;
  for (int k = 0; k < P; ++k)
    for (int r = 0; r < rounds; ++r)
      for (int i = 0; i < N; ++i)
        if (std::fabs(outs[k][r][i] - (i + r) * tri) > 1e-3f) {
          std::fprintf(stderr, "plane: bad sum worker %d round %d idx %d\n", k, r, i);
          return 1;
        }
  return 0;
}

// Three nodes over TCP on 127.0.0.1: master node + two worker nodes.
static int run_tcp(int rounds) {
  const int N = 10, C = 2;
  auto msys = std::make_shared<ActorSystem>("ClusterSystem", ActorSystem::Mode::Threaded, 2);
  std::atomic<bool> done{false};
  MasterParams mp{2, 1.f, 1.f, 1.f, 1, N, rounds - 1, C, false};
  ActorRef master = msys->actor_of(std::make_unique<MasterActor>(mp, [&](int) { done = true; }), "master");
  ClusterConfig mc;
  mc.port = 0;
  mc.roles = {"master"};
  mc.heartbeat_interval_s = 0.05;
  auto mnode = ClusterNode::start(msys, mc);
  mnode->subscribe(master);
  const std::string seed = mnode->address();
  std::vector<std::shared_ptr<ActorSystem>> wsys;
  std::vector<std::shared_ptr<ClusterNode>> wnodes;
  std::atomic<int> outputs{0};
  for (int k = 0; k < 2; ++k) {
    auto s = std::make_shared<ActorSystem>("ClusterSystem", ActorSystem::Mode::Threaded, 2);
    DataSource src = [N](const AllReduceInputRequest& r) {
      std::vector<float> v(N);
      for (int i = 0; i < N; ++i) v[i] = static_cast<float>(i + r.iteration);
      return AllReduceInput{make_host_payload(std::move(v))};
    };
    DataSink sink = [&](const AllReduceOutput&) { outputs++; };
    s->actor_of(std::make_unique<WorkerActor>(src, sink), "worker");
    ClusterConfig wc;
    wc.port = 0;
    wc.roles = {"worker"};
    wc.seed_nodes = {seed};
    wc.heartbeat_interval_s = 0.05;
    wnodes.push_back(ClusterNode::start(s, wc));
    wsys.push_back(s);
  }
  const bool ok = wait_until([&] { return done.load() && outputs.load() >= 2 * rounds; }, 60);
  for (auto& n : wnodes) n->leave();
  for (auto& n : wnodes) n->shutdown();
  mnode->shutdown();
  for (auto& s : wsys) s->shutdown();
  msys->shutdown();
  if (!ok) {
    std::fprintf(stderr, "tcp cluster did not finish (outputs %d)\n", outputs.load());
    return 1;
  }
  return 0;
}

// Lock-free mailbox under contention: producer threads tell numbered messages to one actor
// that stashes everything while "closed" and unstashes when a TextMessage opens it; every
// message must arrive exactly once and in order per producer (Akka's per-pair FIFO).
namespace {
class SeqActor final : public Actor {
 public:
  SeqActor(int producers, std::atomic<int>* total, std::atomic<int>* bad)
      : next_(producers, 0), total_(total), bad_(bad) {}
  void receive(Envelope& env, ActorContext& ctx) override {
    if (auto* t = std::get_if<TextMessage>(&env.msg)) {
      closed_ = t->text == "close";
      if (!closed_) ctx.unstash_all();
      return;
    }
    auto* c = std::get_if<CompleteAllreduce>(&env.msg);
    if (c == nullptr) return;
    if (closed_) {
      ctx.stash(std::move(env));
      return;
    }
    if (c->round != next_[c->srcId]) bad_->fetch_add(1);
    next_[c->srcId] = c->round + 1;
    total_->fetch_add(1);
  }

 private:
  std::vector<int> next_;
  bool closed_ = false;
  std::atomic<int>* total_;
  std::atomic<int>* bad_;
};
}  // namespace

static int run_mailbox(int producers, int per) {
  auto sys = std::make_shared<ActorSystem>("MailboxStress", ActorSystem::Mode::Threaded, 4);
  std::atomic<int> total{0}, bad{0};
  ActorRef a = sys->actor_of(std::make_unique<SeqActor>(producers, &total, &bad), "seq");
  std::vector<std::thread> ts;
  for (int k = 0; k < producers; ++k)
    ts.emplace_back([&, k] {
      for (int i = 0; i < per; ++i) a->tell(CompleteAllreduce{k, i, 0}, nullptr);
    });
  std::thread toggler([&] {  // close / open the actor while the producers run
    for (int i = 0; i < 200; ++i) {
      a->tell(TextMessage{i % 2 == 0 ? "close" : "open"}, nullptr);
      std::this_thread::sleep_for(std::chrono::microseconds(100));
    }
    a->tell(TextMessage{"open"}, nullptr);
  });
  for (auto& t : ts) t.join();
  toggler.join();
  const bool ok = wait_until([&] { return total.load() == producers * per; }, 60.0);
  sys->shutdown();
  if (!ok || bad.load() != 0) {
    std::fprintf(stderr, "mailbox: %d of %d delivered, %d out of order\n", total.load(), producers * per, bad.load());
    return 1;
  }
  return 0;
}

// The akka.tcp front-end (csrc/runtime/akka_endpoint.h): a driver associates and runs every
// round with Java-serialized StartAllreduce by ActorSelection, counting CompleteAllreduce;
// churn threads associate and vanish, send garbage or a frame without a handshake; the
// system shuts down with the driver still associated (the endpoint's stop hook) - the
// endpoint's acceptor / reader / writer threads and the bridge's taps under the sanitizer.
static int run_akka(int P, int N, int C, int rounds) {
  auto sys = std::make_shared<ActorSystem>("ClusterSystem", ActorSystem::Mode::Threaded, 4);
  std::atomic<bool> done{false};
  MasterParams mp{P, 1.f, 1.f, 1.f, 1, N, rounds - 1, C, false};
  mp.externalRounds = true;
  auto actor = std::make_unique<MasterActor>(mp, [&](int) { done = true; });
  auto bridge = ControlBridge::start("127.0.0.1", 0);
  actor->set_bridge(bridge);
  ActorRef master = sys->actor_of(std::move(actor), "master");
  bridge->attach(master, master->path());
  AkkaEndpoint::Options ao;
  ao.heartbeat_s = 0.002;  // heartbeats race the replies on every writer
  auto ep = AkkaEndpoint::start(bridge, ao);
  const int port = ep->port();
  for (int k = 0; k < P; ++k) {
    DataSource src = [N](const AllReduceInputRequest& r) {
      std::vector<float> v(N, static_cast<float>(r.iteration));
      return AllReduceInput{make_host_payload(std::move(v))};
    };
    ActorRef w = sys->actor_of(std::make_unique<WorkerActor>(src, [](const AllReduceOutput&) {}),
                               "worker" + std::to_string(k));
    master->tell(MemberUp{w, "worker", ""}, nullptr);
  }
  auto send_frame = [](int fd, const std::string& pdu) {
    std::string f(4, '\0');
    for (int k = 0; k < 4; ++k) f[static_cast<size_t>(k)] = static_cast<char>(pdu.size() >> (24 - 8 * k));
    f += pdu;
    (void)!::send(fd, f.data(), f.size(), MSG_NOSIGNAL);
  };
  auto read_frame = [](int fd, std::string& body) {
    char h[4];
    size_t got = 0;
    while (got < 4) {
      ssize_t n = ::recv(fd, h + got, 4 - got, 0);
      if (n <= 0) return false;
      got += static_cast<size_t>(n);
    }
    size_t len = 0;
    for (char c : h) len = len << 8 | static_cast<uint8_t>(c);
    body.resize(len);
    got = 0;
    while (got < len) {
      ssize_t n = ::recv(fd, body.data() + got, len - got, 0);
      if (n <= 0) return false;
      got += static_cast<size_t>(n);
    }
    return true;
  };
  akka::Address me;
  me.system = "Driver";
  me.host = "127.0.0.1";
  me.port = 1;
  std::atomic<bool> stop_churn{false};
  std::vector<std::thread> churn;
  for (int t = 0; t < 3; ++t)
    churn.emplace_back([&, t] {
      for (int i = 0; !stop_churn.load(); ++i) {
        int fd = connect_to(port);
        if (fd < 0) continue;
        if ((i + t) % 3 == 0) {
          send_frame(fd, akka::encode_associate(me, 7, ""));
          std::string b;
          (void)read_frame(fd, b);
        } else if ((i + t) % 3 == 1) {
          send_frame(fd, akka::encode_payload_pdu("x"));
        } else {
          (void)!::send(fd, "\xff\xff\xff\xff", 4, MSG_NOSIGNAL);
        }
        ::close(fd);
      }
    });
  std::string err;
  int completed = 0;
  int fd = -1;
  for (int i = 0; i < 100 && fd < 0; ++i) fd = connect_to(port);
  send_frame(fd, akka::encode_associate(me, 42, ""));
  const std::string self = me.str() + "/user/driver";
  auto start = [&](int r) {
    akka::JavaObject o;
    o.class_name = "sample.cluster.allreduce.StartAllreduce";
    o.suid = ep->suid_start();
    o.fields = {{'I', "round", r, 0.0}};
    akka::SerializedMsg inner;
    inner.serializer = akka::kJavaSerializer;
    inner.bytes = akka::java_serialize(o);
    akka::Envelope e;
    e.has_envelope = true;
    e.recipient = ep->address() + "/";
    e.msg.serializer = akka::kContainerSerializer;
    e.msg.bytes = akka::encode_selection(inner, {{1, "user"}, {1, "master"}}, false);
    e.has_sender = true;
    e.sender = self;
    send_frame(fd, akka::encode_payload_pdu(akka::encode_container(e)));
  };
  std::string body;
  int seen = 0;
  auto deadline = std::chrono::steady_clock::now() + std::chrono::seconds(60);
  start(0);
  while (completed < rounds && std::chrono::steady_clock::now() < deadline) {
    if (!read_frame(fd, body)) {
      err = "driver association closed";
      break;
    }
    akka::Pdu pdu;
    akka::Envelope env;
    akka::JavaObject o;
    if (!akka::decode_pdu(body, pdu)) {
      err = "undecodable PDU";
      break;
    }
    if (!pdu.is_payload || !akka::decode_container(pdu.payload, env) || !env.has_envelope) continue;
    if (env.recipient != self || !akka::java_deserialize(env.msg.bytes, o) || o.fields.size() != 2) {
      err = "unexpected message to " + env.recipient;
      break;
    }
    const int round = static_cast<int>(o.fields[0].i);  // fields in stream order: round, srcId
    if (round != completed) continue;
    if (++seen == P) {
      seen = 0;
      if (++completed < rounds) start(completed);
    }
  }
  stop_churn = true;
  for (auto& t : churn) t.join();
  const bool ok = err.empty() && completed == rounds && wait_until([&] { return done.load(); }, 30);
  const auto st = ep->stats();
  sys->await_idle(std::chrono::milliseconds(5000));
  sys->shutdown();  // the master's bridge stop runs the endpoint's stop: the driver is told
  std::string bye;
  akka::Pdu last;
  bool told = false;
  while (read_frame(fd, bye))
    if (akka::decode_pdu(bye, last) && !last.is_payload && last.command == akka::kShuttingDown) told = true;
  ::close(fd);
  bridge.reset();
  ep.reset();
  if (!ok || !told || st.starts != static_cast<uint64_t>(rounds)) {
    std::fprintf(stderr, "akka-driven job failed: %s (rounds %d, starts %llu, shutdown notice %d)\n", err.c_str(),
                 completed, static_cast<unsigned long long>(st.starts), told);
    return 1;
  }
  return 0;
}

// The launch planner (launch_geometry.cc) over pseudo-random shapes: what the kernels rely on
// holds for every geometry that does not throw (and the arithmetic never overflows: UBSan).
static int run_geometry(int iters) {
  uint64_t state = 0x9E3779B97F4A7C15ull;
  auto rnd = [&state](uint64_t lo, uint64_t hi) {  // xorshift64*, fixed seed
    state ^= state >> 12;
    state ^= state << 25;
    state ^= state >> 27;
    return lo + (state * 0x2545F4914F6CDD1Dull >> 11) % (hi - lo + 1);
  };
  int failures = 0, planned = 0;
  auto check = [&](bool ok, const char* what, const char* kind, const GridKnobs& k, int64_t n, int64_t es, int rh) {
    if (ok) return;
    if (failures++ < 10)
      std::fprintf(stderr, "geometry: %s violated (%s world %d grid %d/%d n %lld es %lld ranks_here %d)\n", what, kind,
                   k.world, k.grid, k.default_grid, static_cast<long long>(n), static_cast<long long>(es), rh);
  };
  for (int i = 0; i < iters; ++i) {
    GridKnobs k;
    k.world = static_cast<int>(rnd(1, kMaxRanks));
    k.rows = static_cast<int>(rnd(1, 4));
    k.default_grid = rnd(0, 3) ? 512 : static_cast<int>(rnd(1, 1024));
    k.grid = rnd(0, 1) ? k.default_grid : static_cast<int>(rnd(1, 1024));
    k.size_grid = rnd(0, 3) != 0;
    const int64_t es = rnd(0, 1) ? 2 : 4;
    const SlabLayout L = slab_layout(k.world, int64_t{1} << rnd(16, 28), k.rows - 1, 0, rnd(0, 3) ? 0 : 64, 512 * 1024);
    k.maxch = L.maxch;
    k.slot_bytes = L.slot_bytes;
    k.geom = rnd(0, 1) ? -1 : static_cast<int>(rnd(0, 2));
    k.units_per_wg = rnd(0, 3) ? 0 : static_cast<int>(rnd(1, 8));
    k.sub_max = rnd(0, 3) ? 0 : static_cast<int>(rnd(1, 8));
    k.ring_depth = static_cast<int>(rnd(1, 4));
    k.ring_grid = rnd(0, 1) ? 256 : static_cast<int>(rnd(1, 1024));
    k.th_oneshot_max = rnd(0, 3) ? 256 << 10 : 0;
    const int rh = rnd(0, 1) ? 1 : k.world;
    const int64_t n = static_cast<int64_t>(rnd(1, uint64_t{1} << rnd(1, 31)));
    const int gcap = std::max(1, k.grid / rh);
    auto common = [&](const LaunchGeometry& g, const char* kind, bool rounded, int gx_cap) {
      ++planned;
      check(g.gx >= 1 && g.gx <= gx_cap, "1 <= gx <= grid / ranks_here", kind, k, n, es, rh);
      check(!rounded || (g.chunk * es) % 16 == 0, "chunk a multiple of 16 B", kind, k, n, es, rh);
      check(static_cast<int64_t>(g.nch) * g.chunk >= g.block, "nch * chunk >= block", kind, k, n, es, rh);
      check(static_cast<int64_t>(g.nch) * g.sub <= k.maxch, "nch * sub <= maxch", kind, k, n, es, rh);
      check(g.block * es <= k.slot_bytes + 16, "block fits the slot", kind, k, n, es, rh);
      check(g.sub >= 1 && static_cast<int64_t>(g.sub) * g.subchunk >= g.chunk, "sub * subchunk >= chunk", kind, k, n,
            es, rh);
    };
    static const Algo algos[] = {Algo::OneShot, Algo::TwoShot, Algo::Ring, Algo::RingNative};
    static const char* names[] = {"oneshot", "twoshot", "ring", "ring_native"};
    for (int a = 0; a < 4; ++a) {
      try {
        common(plan_allreduce(algos[a], k, n, es, rh), names[a], true, gcap);
      } catch (const std::logic_error&) {  // does not fit the slab: the caller segments
      }
    }
    try {
      common(plan_allreduce(Algo::TwoShot, k, n, es, rh, true), "adamw", true, gcap);
    } catch (const std::logic_error&) {
    }
    if (n * es <= L.ll_max) {  // the low-latency kernel takes no flags and no S slots
      const LaunchGeometry g = plan_ll(k, n, es, rh);
      ++planned;
      check(g.gx >= 1 && g.gx <= gcap && g.nch == 1 && g.block == n, "ll geometry", "ll", k, n, es, rh);
    }
    const int64_t m = std::min<int64_t>(std::max<int64_t>(16 / es, n / (16 / es) * (16 / es)), k.slot_bytes / es);
    for (int op = 0; op < 3 && k.world > 1; ++op) {
      try {
        LaunchGeometry g = plan_coll(static_cast<Coll>(op), k, m, es, rh);
        g.block = m;
        common(g, "coll", true, gcap);
      } catch (const std::logic_error&) {
      }
    }
    static const float ths[] = {1.f, 0.9f, 0.75f, 0.5f};
    const float thr = ths[rnd(0, 3)], thc = ths[rnd(0, 3)];
    RoundShape spec;
    if (rnd(0, 1) && rh == 1) {
      spec.block = (n + k.world - 1) / k.world;
      spec.chunk = static_cast<int64_t>(rnd(1, uint64_t{1} << rnd(1, 22)));
      spec.order_ref = rnd(0, 1);
      spec.split = rnd(0, 1);
      spec.lag_skip = rnd(0, 1);
    }
    try {
      const ThresholdPlan p = plan_threshold(k, n, es, rh, thr, thc, spec);
      // the one-shot body of a shared launch is sized against the shared-launch cap alone, which
      // an explicit grid lifts (the open one-shot item: plan_threshold's `cap`)
      common(p, "threshold", spec.block == 0, p.oneshot && rh > 1 ? std::max(1, shared_launch_cap(k, rh)) : gcap);
      const int64_t units = static_cast<int64_t>(std::max(1, k.world - 1)) * p.nch * p.sub;
      check((units + p.gx - 1) / p.gx <= kThresholdGatherUnits || k.world == 1, "gather units per workgroup",
            "threshold", k, n, es, rh);
      check(p.min_reduce >= 1 && p.min_reduce <= k.world && p.min_complete >= 0 &&
                p.min_complete <= static_cast<int64_t>(k.world) * p.nch,
            "thresholds within the round", "threshold", k, n, es, rh);
      check(!p.oneshot || (p.full && p.sub == 1 && k.world <= kOneshotRanks), "one-shot body only where it applies",
            "threshold", k, n, es, rh);
      check(!p.lag_skip || (spec.lag_skip && !p.split && p.min_reduce < k.world), "lag skip only where it is safe",
            "threshold", k, n, es, rh);
    } catch (const std::invalid_argument&) {  // does not fit one launch
    }
  }
  if (failures != 0 || planned < iters) {
    std::fprintf(stderr, "geometry: %d violations, %d geometries planned\n", failures, planned);
    return 1;
  }
  return 0;
}

// The copy-engine allreduce's schedule (sdma_schedule.cc) over pseudo-random shapes: what the
// engines (in-order queues, one dependency per copy, signals armed to a count) and the reduce /
// gather kernels (the flag words they wait on) rely on; the arithmetic never overflows (UBSan).
static int run_sdma(int iters) {
  uint64_t state = 0xD1B54A32D192ED03ull;
  auto rnd = [&state](uint64_t lo, uint64_t hi) {  // xorshift64*, fixed seed
    state ^= state >> 12;
    state ^= state << 25;
    state ^= state >> 27;
    return lo + (state * 0x2545F4914F6CDD1Dull >> 11) % (hi - lo + 1);
  };
  int failures = 0;
  int64_t copies = 0;
  for (int it = 0; it < iters; ++it) {
    const int W = static_cast<int>(rnd(0, 3) ? rnd(1, 8) : rnd(1, kSdmaMaxWorld));
    const int64_t es = rnd(0, 1) ? 2 : 4;
    const int64_t slot = sdma_slot_bytes(static_cast<int64_t>((uint64_t{1} << rnd(10, 29)) + (rnd(0, 1) ? rnd(0, 70000) : 0)));
    const int pieces = static_cast<int>(rnd(0, 9)), epp = static_cast<int>(rnd(1, 5)), par = static_cast<int>(rnd(0, 1));
    const int64_t segn = sdma_segment_elems(W, slot, es);
    const int64_t n = rnd(0, 3) == 0 ? segn - static_cast<int64_t>(rnd(0, 1))
                                     : static_cast<int64_t>(rnd(1, std::min<uint64_t>(segn, uint64_t{1} << rnd(0, 34))));
    auto check = [&](bool ok, const char* what, int r) {
      if (ok) return;
      if (failures++ < 10)
        std::fprintf(stderr, "sdma: %s violated (world %d rank %d n %lld es %lld slot %lld pieces %d epp %d par %d)\n",
                     what, W, r, static_cast<long long>(n), static_cast<long long>(es), static_cast<long long>(slot),
                     pieces, epp, par);
    };
    const SdmaSegment g = plan_sdma_segment(W, std::max<int64_t>(n, 1), es, slot, pieces);  // n <= segment: never throws
    const int K = g.K;
    check(K >= 1 && K <= kSdmaMaxPieces && (g.pe * es) % 4096 == 0 && (g.block * es) % 16 == 0, "K, piece alignment", -1);
    check(g.block * es <= slot && g.block * W >= g.n && static_cast<int64_t>(K) * g.pe >= g.block, "blocks cover n in slots", -1);
    const int64_t slab = sdma_slab_bytes(W, slot);
    // flag words each rank's slab receives, over all ranks' schedules
    std::vector<std::vector<int>> written(W, std::vector<int>(2 * kFrWord, 0));
    SdmaSchedule sc;
    for (int r = 0; r < W; ++r) {
      sc = plan_sdma_copies(g, W, r, es, epp, slot, par, std::move(sc));
      copies += static_cast<int64_t>(sc.copies.size());
      std::vector<int64_t> next1(W, 0), next2(W, 0);
      std::vector<int> c1(static_cast<size_t>(W) * K, 0), c2(K, 0), flagged1(static_cast<size_t>(W) * K, 0), flagged2(K, 0);
      int scf = 0, gdf = 0;
      const SdmaCopy* prev = nullptr;
      for (const SdmaCopy& c : sc.copies) {
        const bool flag = c.src == SdmaSrc::Epoch;
        check(c.dst_rank >= 0 && c.dst_rank < W && c.bytes > 0 && c.dst_off >= 0 && c.dst_off + c.bytes <= slab, "inside the slab", r);
        check(c.peer >= 0 && c.peer < W && c.peer != r && c.engine >= 0 && c.engine < epp, "an engine towards a peer", r);
        if (!flag && c.src == SdmaSrc::In) {  // phase 1: block j, in order, to rank j's SD[par][r]
          const int j = c.dst_rank;
          int64_t& at = next1[j];
          const int k = static_cast<int>(at / (g.pe * es));
          check(j != r && c.peer == j && c.src_off == j * g.block * es + at && c.dst_off == sdma_sd_off(W, slot, par, r) + at,
                "phase-1 part continues block j", r);
          check(at % 4096 == 0 && at + c.bytes <= slot && at + c.bytes <= (k + 1) * g.pe * es, "4 KiB aligned inside its piece and slot", r);
          check(c.dep.kind == SdmaSig::Start && c.done.kind == SdmaSig::C1 && c.done.index == j * K + k, "phase-1 signals", r);
          check(flagged1[static_cast<size_t>(j) * K + k] == 0, "no phase-1 part behind its flag", r);
          ++c1[static_cast<size_t>(j) * K + k];
          at += c.bytes;
        } else if (!flag) {  // phase 2: the own block to rank q's RD[par][r]
          const int q = c.dst_rank;
          int64_t& at = next2[q];
          const int k = static_cast<int>(at / (g.pe * es));
          check(q != r && c.peer == q && c.src == SdmaSrc::Out && c.src_off == r * g.block * es + at &&
                    c.dst_off == sdma_rd_off(W, slot, par, r) + at, "phase-2 part continues the own block", r);
          check(at % 4096 == 0 && at + c.bytes <= slot && at + c.bytes <= (k + 1) * g.pe * es, "4 KiB aligned inside its piece and slot", r);
          check(c.dep.kind == SdmaSig::Mid && c.dep.index == k && c.done.kind == SdmaSig::C2 && c.done.index == k, "phase-2 signals", r);
          check(flagged2[k] == 0, "every part of a piece is queued before any of its flags", r);
          ++c2[k];
          at += c.bytes;
        } else {
          check(c.bytes == 4 && c.dst_off % 4 == 0 && c.dst_off + 4 <= kFlagBytes && c.src_off == 0, "a flag word", r);
          ++written[c.dst_rank][static_cast<size_t>(std::min<int64_t>(c.dst_off / 4, 2 * kFrWord - 1))];
          if (c.done.kind == SdmaSig::Scf) {  // FS[r][k] in rank j's slab, behind the piece's last part
            const int j = c.dst_rank, k = c.dep.index % K;
            check(c.dep.kind == SdmaSig::C1 && c.dep.index == j * K + k && c.dst_off == 4 * sdma_fs_word(r, k), "FS flag", r);
            check(prev && prev->src == SdmaSrc::In && prev->done.kind == SdmaSig::C1 && prev->done.index == c.dep.index &&
                      prev->peer == c.peer && prev->engine == c.engine, "FS rides the engine of its piece's last part", r);
            ++flagged1[static_cast<size_t>(c.dep.index)];
            ++scf;
          } else {
            const int k = c.dep.index;
            check(c.done.kind == SdmaSig::Gdf && c.dep.kind == SdmaSig::C2 && k < K && c.dst_off == 4 * sdma_fr_word(r, k), "FR flag", r);
            ++flagged2[k];
            ++gdf;
          }
        }
        prev = &c;
      }
      for (int j = 0; j < W; ++j) {
        check(next1[j] == (j == r ? 0 : sdma_block_len(g.n, g.block, j) * es), "phase 1 tiles block j exactly once", r);
        check(next2[j] == (j == r ? 0 : sdma_block_len(g.n, g.block, r) * es), "phase 2 tiles the own block once per peer", r);
      }
      check(c1 == sc.c1 && c2 == sc.c2 && scf == sc.scf && gdf == sc.gdf, "arm value = copies completing into the signal", r);
      for (int k = 0; k < K; ++k) check(sc.c1[static_cast<size_t>(r) * K + k] == 0, "c1[r, *] = 0", r);
    }
    // the words the kernels of rank t wait on (sdma_reduce_kernel, sdma_gather_kernel)
    for (int t = 0; t < W; ++t) {
      std::vector<int> waited(2 * kFrWord, 0);
      const int64_t rl = sdma_block_len(g.n, g.block, t);
      for (int k = 0; k < K && sdma_block_len(rl, g.pe, k) > 0; ++k)
        for (int s = 0; s < W; ++s)
          if (s != t) ++waited[static_cast<size_t>(sdma_fs_word(s, k))];
      for (int k = 0; k < K && W > 1 && static_cast<int64_t>(k) * g.pe < g.block; ++k)
        for (int s = 0; s < W; ++s)
          if (sdma_block_len(g.n, g.block, s) > static_cast<int64_t>(k) * g.pe) ++waited[static_cast<size_t>(sdma_fr_word(s, k))];
      check(waited == written[t], "the flags sent are the flags the kernels wait on", t);
    }
  }
  if (failures != 0 || copies < iters) {
    std::fprintf(stderr, "sdma: %d violations, %lld copies planned\n", failures, static_cast<long long>(copies));
    return 1;
  }
  // the 4 KiB split on its own
  for (int i = 0; i < 20000; ++i) {
    const int64_t bytes = static_cast<int64_t>(rnd(0, uint64_t{1} << rnd(0, 40)));
    const int epp = static_cast<int>(rnd(1, 16));
    const SdmaParts p = sdma_parts(bytes, epp);
    int64_t at = 0;
    for (int e = 0; e < p.count; ++e) {
      if (p.off(e) != at || at % 4096 != 0 || p.len(e) <= 0) ++failures;
      at += p.len(e);
    }
    if (at != bytes || p.count > epp) ++failures;
  }
  if (failures != 0) std::fprintf(stderr, "sdma: %d split checks failed\n", failures);
  return failures != 0;
}

// The round plane's host bookkeeping (plane_rounds.h): the slot ring and the lock-free hand-off
// between a launching and a completion thread, and the decoding of a finished slot.
static int run_rounds(int records) {
  struct R {
    int seq = 0, slot = 0;
  };
  constexpr int kRing = 4;
  int failures = 0;
  auto check = [&](bool ok, const char* what) {
    if (!ok && failures++ < 10) std::fprintf(stderr, "rounds: %s\n", what);
  };
  {
    RoundQueue<R> q;
    q.reset_slots(kRing);
    { auto dropped = q.take_slot(); }  // a lease dropped without commit returns its slot
    if (q.free_slots() != kRing) {
      std::fprintf(stderr, "rounds: a dropped lease kept its slot\n");
      return 1;
    }
    std::atomic<int> in_flight{0}, max_in_flight{0}, consumed{0};
    std::atomic<int> holder[kRing];
    for (auto& h : holder) h.store(-1);
    std::atomic<bool> fifo{true}, single{true}, ended{false};
    std::thread consumer([&] {
      R r;
      for (int want = 0; q.wait_front(50, &r); ++want) {
        if (r.seq != want) fifo.store(false);
        if (holder[r.slot].exchange(-1) != r.seq) single.store(false);  // the slot was this record's alone
        in_flight.fetch_sub(1);
        consumed.fetch_add(1);
        q.pop_and_release(r.slot);
      }
      ended.store(true);
    });
    uint64_t state = 0x9E3779B97F4A7C15ull;
    for (int i = 0; i < records; ++i) {
      if (i % 64 == 0) {  // the consumer both polls (short pauses) and sleeps (past its 50 us budget)
        state = state * 6364136223846793005ull + 1442695040888963407ull;
        std::this_thread::sleep_for(std::chrono::microseconds((state >> 33) % 201));
      }
      if (i % 97 == 0) {  // and so it does under load
        auto dropped = q.take_slot();
        check(holder[dropped.slot()].load() == -1, "a dropped lease's slot was held by a record");
      }
      auto lease = q.take_slot();
      R r;
      r.seq = i;
      r.slot = lease.slot();
      if (holder[r.slot].exchange(i) != -1) single.store(false);
      const int now = in_flight.fetch_add(1) + 1;
      for (int m = max_in_flight.load(); now > m && !max_in_flight.compare_exchange_weak(m, now);) {
      }
      lease.commit();
      q.push(r);
    }
    q.drain();
    check(consumed.load() == records && q.size() == 0, "drain() returned before the queue was empty");
    check(fifo.load(), "records left the queue out of order");
    check(single.load(), "a slot was held by two records at once");
    check(max_in_flight.load() <= kRing && max_in_flight.load() >= 1, "more records in flight than ring slots");
    check(q.free_slots() == kRing, "a slot was not returned");
    std::this_thread::sleep_for(std::chrono::milliseconds(2));  // past its spin budget: the consumer sleeps
    check(!ended.load(), "the consumer ended before stop()");
    q.stop();
    consumer.join();
    check(ended.load(), "stop() did not end the consumer");
  }
  {
    auto word = [](uint32_t epoch, uint32_t v) { return static_cast<int32_t>((epoch & 0xffffffu) << 8 | v); };
    const uint32_t ep = 0x01000007u;  // the tag is the epoch's low 24 bits
    auto ready = [&](const std::vector<int32_t>& w, size_t counts) {
      size_t from = 0;
      return slot_ready(w.data(), w.size(), counts, ep, &from);
    };
    {  // every tag present, coarse = 1; counts of 0 and of P
      const int P = 3, nch = 2;
      const size_t stride = P * nch + 4;
      std::vector<int32_t> w(stride, 0);
      const int cnt[] = {0, 3, 1, 2, 3, 0};
      for (int i = 0; i < P * nch; ++i) w[i] = word(ep, cnt[i]);
      w[stride - 1] = word(ep, 0x12);
      const SlotResult r = decode_slot(w.data(), stride, P, nch, nch, 1);
      check(ready(w, P * nch) && r.error == 0x12u && r.count == std::vector<int32_t>(cnt, cnt + 6), "decode_slot: plain slot");
      w[2] = word(ep - 1, 1);  // one count still carries the previous epoch's tag
      check(!ready(w, P * nch), "slot_ready: stale count taken as ready");
      w[2] = word(ep, 1);
      w[stride - 1] = 0x12;  // the error word's tag is missing
      check(!ready(w, P * nch), "slot_ready: untagged error word taken as ready");
      size_t from = 0;
      check(!slot_ready(w.data(), stride, P * nch, ep, &from) && from == static_cast<size_t>(P * nch),
            "slot_ready: counts not advanced past their tags");
    }
    {  // coarsened: count[j * 5 + c] = cnt[j * 2 + c / 3]
      const int P = 2, nch = 2, nch_ref = 5, coarse = 3;
      const size_t stride = P * nch + 4;
      std::vector<int32_t> w(stride, 0);
      const int cnt[] = {2, 1, 0, 2};
      for (int i = 0; i < P * nch; ++i) w[i] = word(ep, cnt[i]);
      w[stride - 1] = word(ep, 0);
      const SlotResult r = decode_slot(w.data(), stride, P, nch, nch_ref, coarse);
      check(ready(w, P * nch) && r.error == 0 && r.count == std::vector<int32_t>({2, 2, 2, 1, 1, 0, 0, 0, 2, 2}),
            "decode_slot: coarsened expansion");
    }
  }
  if (failures != 0) std::fprintf(stderr, "rounds: %d checks failed\n", failures);
  return failures != 0;
}

int main(int argc, char** argv) {
  Logger::get().set_level(LogLevel::ERROR);
  const std::string only = argc > 1 ? argv[1] : "";
  int rc = 0;
  if (only.empty() || only == "geometry") rc = run_geometry(4000);
  if (rc == 0 && (only.empty() || only == "sdma")) rc = run_sdma(1500);
  if (rc == 0 && (only.empty() || only == "rounds")) rc = run_rounds(5000);
  if (rc == 0 && (only.empty() || only == "mailbox")) rc = run_mailbox(6, 20000);
  if (rc == 0 && (only.empty() || only == "local")) rc = run_local(4, 37, 3, 30);
  if (rc == 0 && (only.empty() || only == "local2")) rc = run_local(3, 9, 2, 30);
  if (rc == 0 && (only.empty() || only == "tcp")) rc = run_tcp(20);
  if (rc == 0 && (only.empty() || only == "plane")) rc = run_plane(3, 41, 4, 40);
  if (rc == 0 && (only.empty() || only == "bridge")) rc = run_bridge(3, 23, 4, 60);
  if (rc == 0 && (only.empty() || only == "bridge_teardown")) rc = run_bridge_teardown(3, 23, 4, 400);
  if (rc == 0 && (only.empty() || only == "akka")) rc = run_akka(3, 23, 4, 60);
  std::printf(rc == 0 ? "runtime_stress: OK\n" : "runtime_stress: FAILED\n");
  return rc;
}
