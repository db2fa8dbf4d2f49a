// jit.hip — the run-time compiler of libmlgpu.so: hiprtc (looked up at run time), the memory and disk caches of generated code
// objects, module loading, and the fused kernels of processor chains without an ahead-of-time instantiation (mlgpu_jit_chain).
// graph.hip generates the graph kernels' sources and hands them here (the interface is in mlgpu_internal.hpp).
#include <hip/hiprtc.h>  // (types and enumerators only: the library is looked up at run time, see Hiprtc below)
#include <dlfcn.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <fcntl.h>
#include <sys/file.h>
#include <sys/stat.h>
#include <unistd.h>

#include <chrono>
#include <map>
#include <mutex>
#include <sstream>

#include "mlgpu_internal.hpp"

extern const char mlgpu_device_source_hash_str[];
extern const int mlgpu_embedded_count;
extern const char* const mlgpu_embedded_names[];
extern const char* const mlgpu_embedded_sources[];

namespace
{
struct CompiledModule
{
  hipModule_t module{nullptr};
  std::map<std::string, hipFunction_t> fns;
};

std::mutex g_cacheMutex;
std::map<std::string, CompiledModule> g_cache;  // key: device id + source

// The options every run-time kernel is compiled with (part of the disk cache's key): the ahead-of-time build's own
// (csrc/Makefile) apart from its scheduling strategy, max-ilp (profiles/archive/r03_jit_maxilp.txt: what it does to config 5).
const std::vector<std::string>& jitOptions()
{
  static const std::vector<std::string> opts = {"--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-fno-slp-vectorize"};
  return opts;
}

// hiprtc, looked up at RUN TIME (round 6): libmlgpu.so does not link it, so an installation without the compiler still loads and
// runs every ahead-of-time kernel, and every generated one whose code it is given (the disk cache, mlgpu_jit_cache_import). A
// graph or chain that needs a compile there fails with MLGPU_ERR_UNSUPPORTED and says why. MLGPU_HIPRTC=off: behave as if the
// library were absent (what tests/test_abi.py uses); MLGPU_HIPRTC=<path>: that library.
struct Hiprtc
{
  void* lib{nullptr};
  decltype(&::hiprtcCreateProgram) createProgram{nullptr};
  decltype(&::hiprtcCompileProgram) compileProgram{nullptr};
  decltype(&::hiprtcGetProgramLogSize) getProgramLogSize{nullptr};
  decltype(&::hiprtcGetProgramLog) getProgramLog{nullptr};
  decltype(&::hiprtcGetCodeSize) getCodeSize{nullptr};
  decltype(&::hiprtcGetCode) getCode{nullptr};
  decltype(&::hiprtcDestroyProgram) destroyProgram{nullptr};
  decltype(&::hiprtcGetErrorString) getErrorString{nullptr};
  decltype(&::hiprtcVersion) version{nullptr};
  std::string why;
  Hiprtc()
  {
    const char* knob = getenv("MLGPU_HIPRTC");
    for (const char* name : {knob && strcmp(knob, "off") ? knob : "libhiprtc.so", "libhiprtc.so.7", "/opt/rocm/lib/libhiprtc.so"})
    {
      lib = dlopen(name, RTLD_NOW | RTLD_LOCAL);
      if (lib) break;
    }
    if (!lib)
    {
      why = std::string("libhiprtc.so cannot be loaded (") + (dlerror() ? dlerror() : "not found") + ")";
      return;
    }
#define MLGPU_RTC_SYM(member, symbol) member = (decltype(member))dlsym(lib, #symbol)
    MLGPU_RTC_SYM(createProgram, hiprtcCreateProgram);
    MLGPU_RTC_SYM(compileProgram, hiprtcCompileProgram);
    MLGPU_RTC_SYM(getProgramLogSize, hiprtcGetProgramLogSize);
    MLGPU_RTC_SYM(getProgramLog, hiprtcGetProgramLog);
    MLGPU_RTC_SYM(getCodeSize, hiprtcGetCodeSize);
    MLGPU_RTC_SYM(getCode, hiprtcGetCode);
    MLGPU_RTC_SYM(destroyProgram, hiprtcDestroyProgram);
    MLGPU_RTC_SYM(getErrorString, hiprtcGetErrorString);
    MLGPU_RTC_SYM(version, hiprtcVersion);
#undef MLGPU_RTC_SYM
    if (!createProgram || !compileProgram || !getProgramLogSize || !getProgramLog || !getCodeSize || !getCode || !destroyProgram || !getErrorString)
    {
      why = "libhiprtc.so lacks an entry point this library uses";
      dlclose(lib);
      lib = nullptr;
    }
  }
};
// nullptr (and `why`) where the compiler is not there - or a test says so
const Hiprtc* hiprtc(std::string* why = nullptr)
{
  static const Hiprtc rtc;
  const char* knob = getenv("MLGPU_HIPRTC");
  if (knob && !strcmp(knob, "off"))
  {
    if (why) *why = "run-time compilation is switched off (MLGPU_HIPRTC=off)";
    return nullptr;
  }
  if (!rtc.lib)
  {
    if (why) *why = rtc.why;
    return nullptr;
  }
  return &rtc;
}

// compile `source` for gfx950 and load it on the current device; returns nullptr and fills `log` on failure
bool compileToCode(const std::string& source, std::vector<char>& code, std::string& log)
{
  hiprtcProgram prog;
  code.clear();
  std::string why;
  const Hiprtc* rtc = hiprtc(&why);
  if (!rtc)
  {
    log = "this kernel is not in the memory or disk cache and " + why + ": compile it where hiprtc is installed and bring its code along (mlgpu_jit_cache_export / _import)";
    return false;
  }
  if (rtc->createProgram(&prog, source.c_str(), "mlgpu_jit.hip", mlgpu_embedded_count, (const char**)mlgpu_embedded_sources,
                          (const char**)mlgpu_embedded_names) != HIPRTC_SUCCESS)
  {
    log = "hiprtcCreateProgram failed";
    return false;
  }
  std::vector<const char*> opts;
  for (const std::string& o : jitOptions()) opts.push_back(o.c_str());
  const hiprtcResult r = rtc->compileProgram(prog, (int)opts.size(), opts.data());
  size_t logSize = 0;
  rtc->getProgramLogSize(prog, &logSize);
  if (logSize > 1)
  {
    log.resize(logSize);
    rtc->getProgramLog(prog, &log[0]);
  }
  size_t codeSize = 0;
  if (r == HIPRTC_SUCCESS) rtc->getCodeSize(prog, &codeSize);
  if (codeSize)
  {
    code.resize(codeSize);
    rtc->getCode(prog, code.data());
  }
  rtc->destroyProgram(&prog);
  if (r != HIPRTC_SUCCESS && log.empty()) log = rtc->getErrorString(r);
  return r == HIPRTC_SUCCESS && codeSize > 0;
}

// hiprtc results by source. Two levels: in memory (identical graphs and the size probe of graph_compile compile once per
// process) and on disk (a process that starts again - a plug-in host reloading, the next benchmark run - finds the code
// object of every graph it has built before and skips hiprtc, which takes 0.3-2 s per kernel). The disk key is a hash of
// everything that decides the code object: the generated source, the compile options, every embedded device header and
// the hiprtc version. Files are written to a temporary name and renamed, so concurrent processes (one rank per GPU) can
// share the directory. MLGPU_CACHE_DIR names it (default $XDG_CACHE_HOME/mlgpu or ~/.cache/mlgpu); MLGPU_CACHE_DIR=off
// disables the disk level.
std::mutex g_codeMutex;
std::map<std::string, std::vector<char>> g_codeCache;
struct JitStats
{
  uint64_t compiles{0}, diskHits{0}, memoryHits{0}, diskWrites{0};
  double compileSeconds{0}, diskLoadSeconds{0};
} g_jitStats;

uint64_t fnv1a(uint64_t h, const void* data, size_t n)
{
  const unsigned char* p = (const unsigned char*)data;
  for (size_t i = 0; i < n; ++i) h = (h ^ p[i]) * 0x100000001b3ull;
  return h;
}

// The cache directory, or "" when the disk level is off or the directory cannot be trusted: code objects are loaded into
// the GPU as they are, so the directory must belong to this user and be writable by nobody else (a directory another user
// can write to would let them choose the code this process runs).
std::string cacheDir()
{
  const char* d = getenv("MLGPU_CACHE_DIR");
  if (d && !strcmp(d, "off")) return "";
  std::string dir;
  if (d && *d)
    dir = d;
  else if (const char* x = getenv("XDG_CACHE_HOME"))
    dir = std::string(x) + "/mlgpu";
  else if (const char* h = getenv("HOME"))
    dir = std::string(h) + "/.cache/mlgpu";
  else
    return "";
  // mkdir -p; what we create is ours alone
  for (size_t i = 1; i <= dir.size(); ++i)
    if (i == dir.size() || dir[i] == '/') mkdir(dir.substr(0, i).c_str(), 0700);
  struct stat st;
  if (stat(dir.c_str(), &st) != 0 || !S_ISDIR(st.st_mode)) return "";
  if (st.st_uid != geteuid() || (st.st_mode & (S_IWGRP | S_IWOTH)))
  {
    fprintf(stderr, "mlgpu: kernel cache directory %s is not owned by this user or is writable by others: disk cache off\n", dir.c_str());
    return "";
  }
  return dir;
}

// Everything that decides a code object besides the generated source: compile options, the fingerprint of the device
// headers of this build (embed.py: the headers hiprtc is given are part of it), the HIP runtime / hiprtc versions with
// their patch level, and the library's ABI version.
const std::string& cacheContext()
{
  static const std::string ctx = [] {
    std::string c = "mlgpu-kernel-cache 2\n";
    for (const std::string& o : jitOptions()) c += o + " ";
    c += "\ndevice-sources " + std::string(mlgpu_device_source_hash_str);
    int major = 0, minor = 0, runtime = 0, driver = 0;
    if (const Hiprtc* rtc = hiprtc())
      if (rtc->version) rtc->version(&major, &minor);  // (0.0 without the compiler: such a process only ever READS code it is given)
    if (hipRuntimeGetVersion(&runtime) != hipSuccess) runtime = -1;
    if (hipDriverGetVersion(&driver) != hipSuccess) driver = -1;
    c += "\nhiprtc " + std::to_string(major) + "." + std::to_string(minor) + " runtime " + std::to_string(runtime) + " driver " + std::to_string(driver);
#ifdef HIP_VERSION_GITHASH
    c += std::string(" built-with ") + HIP_VERSION_GITHASH;
#endif
    c += "\nabi " + std::to_string(MLGPU_ABI_VERSION) + "\n";
    return c;
  }();
  return ctx;
}

std::string cacheFile(const std::string& source)
{
  // (looked up again whenever MLGPU_CACHE_DIR changes: a host - or a test - may switch the disk level off after the first kernel)
  static std::mutex m;
  static std::string dirFor, dirValue;
  static bool dirKnown = false;
  std::string dir;
  {
    std::lock_guard<std::mutex> lock(m);
    const char* envNow = getenv("MLGPU_CACHE_DIR");
    const std::string key = envNow ? envNow : "";
    if (!dirKnown || key != dirFor)
    {
      dirValue = cacheDir();
      dirFor = key;
      dirKnown = true;
    }
    dir = dirValue;
  }
  if (dir.empty()) return "";
  const std::string& ctx = cacheContext();
  uint64_t h = 0xcbf29ce484222325ull;
  h = fnv1a(h, ctx.data(), ctx.size());
  h = fnv1a(h, source.data(), source.size());
  char name[64];
  snprintf(name, sizeof(name), "/%016llx-%zu.co", (unsigned long long)h, source.size());
  return dir + name;
}

// A cache file = header line "MLGPUCO2 <context bytes> <source bytes> <code bytes>\n", the context, the generated source,
// the code object. The file name is only a 64-bit hash: a file is used when its context and its source are byte for byte
// the ones asked for, so neither a hash collision nor another compiler / library build can hand back a different kernel.
bool readCacheFile(const std::string& path, const std::string& source, std::vector<char>& code)
{
  FILE* f = fopen(path.c_str(), "rb");
  if (!f) return false;
  bool ok = false;
  char magic[16] = {0};
  unsigned long long nCtx = 0, nSrc = 0, nCode = 0;
  const std::string& ctx = cacheContext();
  if (fscanf(f, "%15s %llu %llu %llu", magic, &nCtx, &nSrc, &nCode) == 4 && fgetc(f) == '\n' && !strcmp(magic, "MLGPUCO2") &&
      nCtx == ctx.size() && nSrc == source.size() && nCode > 64 && nCode < (1ull << 30))
  {
    std::string gotCtx(nCtx, '\0'), gotSrc(nSrc, '\0');
    code.resize((size_t)nCode);
    ok = fread(&gotCtx[0], 1, nCtx, f) == nCtx && fread(&gotSrc[0], 1, nSrc, f) == nSrc && fread(code.data(), 1, (size_t)nCode, f) == (size_t)nCode &&
         fgetc(f) == EOF && gotCtx == ctx && gotSrc == source && !memcmp(code.data(), "\177ELF", 4);
  }
  fclose(f);
  if (!ok) code.clear();
  return ok;
}

bool writeCacheFile(const std::string& path, const std::string& source, const std::vector<char>& code)
{
  // a temporary file of our own in the same directory (mkstemp: unique whatever shares the directory - other processes,
  // containers with the same pids, hosts on a network file system), then an atomic rename
  std::string tmp = path + ".XXXXXX";
  const int fd = mkstemp(&tmp[0]);
  if (fd < 0) return false;
  FILE* f = fdopen(fd, "wb");
  if (!f)
  {
    close(fd);
    remove(tmp.c_str());
    return false;
  }
  const std::string& ctx = cacheContext();
  bool ok = fprintf(f, "MLGPUCO2 %zu %zu %zu\n", ctx.size(), source.size(), code.size()) > 0;
  ok = ok && fwrite(ctx.data(), 1, ctx.size(), f) == ctx.size() && fwrite(source.data(), 1, source.size(), f) == source.size() &&
       fwrite(code.data(), 1, code.size(), f) == code.size();
  ok = (fclose(f) == 0) && ok;
  if (ok && rename(tmp.c_str(), path.c_str()) == 0) return true;
  remove(tmp.c_str());
  return false;
}

}  // namespace

bool mlgpu_jit_code(const std::string& source, std::vector<char>& code, std::string& log)
{
  auto inMemory = [&] {
    std::lock_guard<std::mutex> lock(g_codeMutex);
    auto it = g_codeCache.find(source);
    if (it == g_codeCache.end()) return false;
    code = it->second;
    ++g_jitStats.memoryHits;
    return true;
  };
  if (inMemory()) return true;
  // One build at a time: the host threads of a DeviceGroup ask for the same kernels at the same moment, and the second one
  // should find the first one's result instead of running hiprtc again beside it.
  static std::mutex buildMutex;
  std::lock_guard<std::mutex> building(buildMutex);
  if (inMemory()) return true;
  const std::string path = cacheFile(source);
  bool fromDisk = false;
  // One build per MACHINE too: the ranks of a multi-GPU job start together and all ask for the same kernel. Whoever gets
  // the advisory lock on <entry>.lock first compiles and writes the entry; the others block in flock(), then find it. The
  // kernel drops the lock when its holder dies, so a killed rank cannot strand the rest.
  struct FileLock
  {
    int fd{-1};
    explicit FileLock(const std::string& p)
    {
      if (p.empty()) return;
      fd = open((p + ".lock").c_str(), O_CREAT | O_RDWR | O_CLOEXEC, 0600);
      if (fd >= 0 && flock(fd, LOCK_EX) != 0)
      {
        close(fd);
        fd = -1;
      }
    }
    ~FileLock()
    {
      if (fd >= 0)
      {
        flock(fd, LOCK_UN);
        close(fd);
      }
    }
  } entryLock(path);
  if (!path.empty())
  {
    const auto t0 = std::chrono::steady_clock::now();
    fromDisk = readCacheFile(path, source, code);  // anything else under that name (a truncated write, another build's file) is ignored and rebuilt
    if (fromDisk)
    {
      std::lock_guard<std::mutex> lock(g_codeMutex);
      ++g_jitStats.diskHits;
      g_jitStats.diskLoadSeconds += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    }
  }
  if (!fromDisk)
  {
    const auto t0 = std::chrono::steady_clock::now();
    if (!compileToCode(source, code, log)) return false;
    {
      std::lock_guard<std::mutex> lock(g_codeMutex);
      ++g_jitStats.compiles;
      g_jitStats.compileSeconds += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    }
    if (!path.empty() && writeCacheFile(path, source, code))
    {
      std::lock_guard<std::mutex> lock(g_codeMutex);
      ++g_jitStats.diskWrites;
    }
  }
  std::lock_guard<std::mutex> lock(g_codeMutex);
  g_codeCache[source] = code;
  return true;
}

static CompiledModule* compileAndLoad(int device, const std::string& source, std::string& log)
{
  const std::string key = std::to_string(device) + "\n" + source;
  {
    std::lock_guard<std::mutex> lock(g_cacheMutex);
    auto it = g_cache.find(key);
    if (it != g_cache.end()) return &it->second;
  }
  // hiprtc (seconds, on a compile job's worker thread) runs OUTSIDE the module cache's lock: a thread that only looks a loaded module
  // up - an autotune trial inside graph_process, a bank's chain, another graph - never waits for someone else's compile
  std::vector<char> code;
  if (!mlgpu_jit_code(source, code, log)) return nullptr;

  std::lock_guard<std::mutex> lock(g_cacheMutex);
  auto it = g_cache.find(key);  // (another thread may have loaded the same source meanwhile)
  if (it != g_cache.end()) return &it->second;
  CompiledModule cm;
  const hipError_t e = hipModuleLoadData(&cm.module, code.data());
  if (e != hipSuccess)
  {
    log = std::string("hipModuleLoadData: ") + hipGetErrorString(e);
    return nullptr;
  }
  return &(g_cache[key] = cm);
}

// compile only (no device needed): used by mlgpu_jit_selftest
bool mlgpu_jit_compile_only(const std::string& source, std::string& log)
{
  std::vector<char> code;
  return compileToCode(source, code, log);
}

static hipFunction_t getFunction(CompiledModule* cm, const char* name, std::string& log)
{
  auto it = cm->fns.find(name);
  if (it != cm->fns.end()) return it->second;
  hipFunction_t f = nullptr;
  const hipError_t e = hipModuleGetFunction(&f, cm->module, name);
  if (e != hipSuccess)
  {
    log = std::string("hipModuleGetFunction(") + name + "): " + hipGetErrorString(e);
    return nullptr;
  }
  cm->fns[name] = f;
  return f;
}

hipFunction_t mlgpu_jit_function(int device, const std::string& source, const char* name, std::string& log, bool* loaded)
{
  CompiledModule* cm = compileAndLoad(device, source, log);
  if (loaded) *loaded = cm != nullptr;
  return cm ? getFunction(cm, name, log) : nullptr;
}

hipError_t mlgpu_jit_launch(hipFunction_t fn, void* args, size_t argBytes, size_t V, hipStream_t stream)
{
  void* config[] = {HIP_LAUNCH_PARAM_BUFFER_POINTER, args, HIP_LAUNCH_PARAM_BUFFER_SIZE, &argBytes, HIP_LAUNCH_PARAM_END};
  const unsigned blocks = (unsigned)((V + 255) / 256);
  return hipModuleLaunchKernel(fn, blocks, 1, 1, 256, 1, 1, 0, stream, nullptr, config);
}

// Registers and scratch bytes per lane of the (only) kernel of a code object, read from its metadata note (msgpack: the key
// string, then an unsigned integer).
bool mlgpu_jit_code_number(const std::vector<char>& code, const char* key, long& value)
{
  const size_t klen = strlen(key);
  for (size_t i = 0; i + klen + 1 < code.size(); ++i)
  {
    if (memcmp(code.data() + i, key, klen) != 0) continue;
    const unsigned char* p = (const unsigned char*)code.data() + i + klen;
    const size_t left = code.size() - (i + klen);
    if (p[0] <= 0x7f) { value = p[0]; return true; }
    if (p[0] == 0xcc && left >= 2) { value = p[1]; return true; }
    if (p[0] == 0xcd && left >= 3) { value = (p[1] << 8) | p[2]; return true; }
    if (p[0] == 0xce && left >= 5) { value = ((long)p[1] << 24) | (p[2] << 16) | (p[3] << 8) | p[4]; return true; }
  }
  return false;
}

// ---- fused kernels for processor chains without an ahead-of-time instantiation -------------------
// Generates `chain_kernel_body<Chain<kinds...>, HAS_SIGNAL>` wrappers; used by mlgpu_bank_create. mix: the form of the chain that
// sums its voices inside the kernel (chain_kernel_body<CH, HAS_SIGNAL, true>, mlgpu_bank_prepare_mixdown), generated on request for
// the chains chains.hip has no ahead-of-time instantiation of.
std::string mlgpu_jit_chain_source(const int32_t* kinds, int n, bool strictSvf, bool mix)
{
  std::ostringstream s;
  s << "// generated by libmlgpu graph.hip (chain" << (mix ? ", voices summed in the kernel" : "") << ")\n" << (strictSvf ? "#define MLGPU_SVF_STRICT 1\n" : "")
    << "#include \"mldsp_kernels.hpp\"\nusing namespace mldev;\n";
  // a plain cascade of 2, 4 or 8 equal SVF sections keeps its stage-skewed form (one lane per channel; chains.hip picks wider
  // forms by bank size for the ahead-of-time kernels): strict mode must not cost config 4 its kernel
  bool cascade = !mix && (n == 2 || n == 4 || n == 8) && (kinds[0] == MLGPU_PROC_LOPASS || kinds[0] == MLGPU_PROC_HIPASS || kinds[0] == MLGPU_PROC_BANDPASS);
  for (int i = 1; i < n; ++i) cascade = cascade && kinds[i] == kinds[0];
  if (cascade)
  {
    for (int sig = 1; sig >= 0; --sig)
      s << "extern \"C\" __global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2))) void mlgpu_chain_" << (sig ? "signal" : "const")
        << "(const ChainArgs a) { cascade_lanes_body<" << kinds[0] << ", " << n << ", 1, 8, " << (sig ? "true" : "false") << ">(a); }\n";
    return s.str();
  }
  s << "using CH = Chain<";
  for (int i = 0; i < n; ++i) s << (i ? ", " : "") << kinds[i];
  s << ">;\n";
  for (int sig = 1; sig >= 0; --sig)
    s << "extern \"C\" __global__ __launch_bounds__(256) void mlgpu_chain_" << (mix ? "mix_" : "") << (sig ? "signal" : "const") << "(const ChainArgs a) { chain_kernel_body<CH, "
      << (sig ? "true" : "false") << (mix ? ", true" : "") << ">(a); }\n";
  return s.str();
}

static bool jitChain(mlgpu_engine* e, const int32_t* kinds, int n, bool mix, void** fnSignal, void** fnConst, std::string& log)
{
  CompiledModule* cm = compileAndLoad(e->device, mlgpu_jit_chain_source(kinds, n, e->strictSvf, mix), log);
  if (!cm) return false;
  *fnSignal = (void*)getFunction(cm, mix ? "mlgpu_chain_mix_signal" : "mlgpu_chain_signal", log);
  *fnConst = (void*)getFunction(cm, mix ? "mlgpu_chain_mix_const" : "mlgpu_chain_const", log);
  return *fnSignal && *fnConst;
}

bool mlgpu_jit_chain(mlgpu_engine* e, const int32_t* kinds, int n, void** fnSignal, void** fnConst, std::string& log) { return jitChain(e, kinds, n, false, fnSignal, fnConst, log); }
bool mlgpu_jit_chain_mix(mlgpu_engine* e, const int32_t* kinds, int n, void** fnSignal, void** fnConst, std::string& log) { return jitChain(e, kinds, n, true, fnSignal, fnConst, log); }
hipError_t mlgpu_jit_chain_launch(void* fn, const ChainArgs& a, hipStream_t stream)
{
  ChainArgs copy = a;  // (the launch takes a mutable argument buffer)
  return mlgpu_jit_launch((hipFunction_t)fn, &copy, sizeof(copy), a.V, stream);
}

extern "C"
{
  // Every generated kernel this process holds (compiled here or read from the disk cache), as one relocatable blob: what an
  // installation WITHOUT hiprtc is given so that its graphs and chains find their code. Header: magic, the fingerprint of the device
  // headers the kernels were generated from (a bundle of another build is refused: its kernels would be looked up by other sources
  // anyway), count; then per kernel the generated source (the key) and the code object.
  static const char kBundleMagic[8] = {'M', 'L', 'G', 'P', 'U', 'K', 'B', '1'};
  int mlgpu_jit_cache_export(void* buffer, size_t capacity, size_t* needed)
  {
    std::lock_guard<std::mutex> lock(g_codeMutex);
    const std::string fp = mlgpu_device_source_hash_str;
    size_t total = sizeof(kBundleMagic) + 8 + fp.size() + 8;
    for (const auto& kv : g_codeCache) total += 16 + kv.first.size() + kv.second.size();
    if (needed) *needed = total;
    if (!buffer) return MLGPU_OK;
    if (capacity < total) return MLGPU_ERR_RANGE;
    char* p = (char*)buffer;
    auto put = [&p](const void* src, size_t n) {
      memcpy(p, src, n);
      p += n;
    };
    auto put64 = [&put](uint64_t v) { put(&v, 8); };
    put(kBundleMagic, sizeof(kBundleMagic));
    put64(fp.size());
    put(fp.data(), fp.size());
    put64(g_codeCache.size());
    for (const auto& kv : g_codeCache)
    {
      put64(kv.first.size());
      put64(kv.second.size());
      put(kv.first.data(), kv.first.size());
      put(kv.second.data(), kv.second.size());
    }
    return MLGPU_OK;
  }
  int mlgpu_jit_cache_import(const void* buffer, size_t size, size_t* kernels)
  {
    if (kernels) *kernels = 0;
    if (!buffer) return MLGPU_ERR_INVALID;
    const char *p = (const char*)buffer, *end = p + size;
    auto get64 = [&p, end](uint64_t& v) {
      if ((size_t)(end - p) < 8) return false;
      memcpy(&v, p, 8);
      p += 8;
      return true;
    };
    if (size < sizeof(kBundleMagic) || memcmp(p, kBundleMagic, sizeof(kBundleMagic)) != 0) return MLGPU_ERR_INVALID;
    p += sizeof(kBundleMagic);
    uint64_t n = 0;
    if (!get64(n) || (size_t)(end - p) < n) return MLGPU_ERR_INVALID;
    if (std::string(p, (size_t)n) != mlgpu_device_source_hash_str) return MLGPU_ERR_UNSUPPORTED;  // kernels of another build of the device code
    p += n;
    uint64_t count = 0;
    if (!get64(count)) return MLGPU_ERR_INVALID;
    std::vector<std::pair<std::string, std::vector<char>>> items;
    for (uint64_t i = 0; i < count; ++i)
    {
      uint64_t ns = 0, nc = 0;
      if (!get64(ns) || !get64(nc) || (size_t)(end - p) < ns || (size_t)(end - p) - ns < nc) return MLGPU_ERR_INVALID;
      if (nc < 4 || memcmp(p + ns, "\x7f" "ELF", 4) != 0) return MLGPU_ERR_INVALID;  // (what goes to the module loader is at least an ELF file)
      items.emplace_back(std::string(p, (size_t)ns), std::vector<char>(p + ns, p + ns + nc));
      p += ns + nc;
    }
    std::lock_guard<std::mutex> lock(g_codeMutex);
    for (auto& it : items) g_codeCache[it.first] = std::move(it.second);
    if (kernels) *kernels = items.size();
    return MLGPU_OK;
  }
  // (tests) forget the kernels held in memory: the next request goes to the disk cache or the compiler again
  int mlgpu_jit_cache_clear_memory(void)
  {
    std::lock_guard<std::mutex> lock(g_codeMutex);
    g_codeCache.clear();
    return MLGPU_OK;
  }
  // 1 where run-time compilation is there (libhiprtc.so can be loaded and MLGPU_HIPRTC is not "off"), else 0
  int mlgpu_jit_compiler_available(void) { return hiprtc() ? 1 : 0; }

  int mlgpu_jit_stats(uint64_t* compiles, uint64_t* diskHits, uint64_t* memoryHits, double* compileSeconds, double* diskLoadSeconds)
  {
    std::lock_guard<std::mutex> lock(g_codeMutex);
    if (compiles) *compiles = g_jitStats.compiles;
    if (diskHits) *diskHits = g_jitStats.diskHits;
    if (memoryHits) *memoryHits = g_jitStats.memoryHits;
    if (compileSeconds) *compileSeconds = g_jitStats.compileSeconds;
    if (diskLoadSeconds) *diskLoadSeconds = g_jitStats.diskLoadSeconds;
    return MLGPU_OK;
  }
}
