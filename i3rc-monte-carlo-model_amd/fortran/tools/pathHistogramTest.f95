! The path-length histogram through the Fortran shell: specifyParameters(pathHistogramEdges = edges) and reportResults(pathHistogramUp =,
! pathHistogramPathUp =, pathHistogramDown =, pathHistogramPathDown =) on pathLengthTest's small cloud over a reflecting surface.
! Prints the four arrays, bin after bin with the overflow bin last, and what they are for: for three absorption coefficients k the
! reflectance ratio R(k) / R(0) = sum_b up_b exp(-k Lbar_b) / sum_b up_b, Lbar_b = pathUp_b / up_b the bin's mean path, summed in double
! precision (tests/test_gpu_path_histogram.py runs the same photons through the Python mirror) -- and what the shell answers when the
! arrays are asked for without having been computed, into an array of the wrong size, or with bad edges.
program pathHistogramTest
  use ErrorMessages
  use RandomNumbers
  use scatteringPhaseFunctions
  use opticalProperties
  use monteCarloIllumination
  use monteCarloRadiativeTransfer
  implicit none
  integer, parameter :: nx = 4, ny = 2, nz = 6, nPhotons = 50000, nBins = 24
  real,    parameter :: absorption(3) = (/ 1.e-5, 1.e-4, 1.e-3 /)
  type(ErrorMessage)         :: status
  type(domain)               :: cloud
  type(integrator)           :: mc
  type(randomNumberSequence) :: randoms
  type(photonStream)         :: photons
  type(phaseFunction)        :: hg
  type(phaseFunctionTable)   :: table
  real    :: ext(nx, ny, nz), ssa(nx, ny, nz), edges(nBins + 1), bad(nBins + 1)
  real    :: up(nBins + 1), pathUp(nBins + 1), down(nBins + 1), pathDown(nBins + 1), wrong(nBins)
  double precision :: ratio(3), total
  integer :: idx(nx, ny, nz), i, j, k, b

  hg = new_PhaseFunction(0.85**(/ (i, i = 1, 64) /), status = status)
  table = new_PhaseFunctionTable((/ hg /), key = (/ 1. /), status = status)
  do k = 1, nz
    do j = 1, ny
      do i = 1, nx
        ext(i, j, k) = 0.0002
        if(k >= 3 .and. k <= 5) ext(i, j, k) = 0.004 * (1 + mod(i + j, 3))
      end do
    end do
  end do
  ssa = 0.95; idx = 1
  cloud = new_Domain((/ 0., 500., 1000., 1500., 2000. /), (/ 0., 500., 1000. /), (/ 0., 100., 250., 300., 500., 800., 1000. /), status)
  call addOpticalComponent(cloud, "cloud", ext, ssa, idx, table, status = status)
  mc = new_Integrator(cloud, status)
  if(stateIsFailure(status)) then
    print *, "new_Integrator failed"; stop 1
  end if
  call specifyParameters(mc, surfaceAlbedo = 0.3, minInverseTableSize = 10001, status = status)
  ! edges in geometric progression from half the domain's depth
  edges(1) = 0.; edges(2) = 500.
  do b = 3, nBins + 1
    edges(b) = edges(b - 1) * 1.25
  end do

  ! asked for before it is switched on
  randoms = new_RandomNumberSequence(seed = (/ 7, 3 /))
  photons = new_PhotonStream(0.5, 30., numberOfPhotons = nPhotons, randomNumbers = randoms, status = status)
  call computeRadiativeTransfer(mc, randoms, photons, status)
  call finalize_PhotonStream(photons)
  call initializeState(status)
  call reportResults(mc, status = status, pathHistogramUp = up)
  print '(a, l2, 1x, a)', "unavailable ", stateIsFailure(status), trim(failureText())
  call initializeState(status)

  ! bad edges are refused by name
  bad = edges; bad(5) = bad(4)
  call specifyParameters(mc, status = status, pathHistogramEdges = bad)
  print '(a, l2, 1x, a)', "badedges    ", stateIsFailure(status), trim(failureText())
  call initializeState(status)

  call specifyParameters(mc, status = status, pathHistogramEdges = edges)
  if(stateIsFailure(status)) then
    print *, "specifyParameters(pathHistogramEdges) failed: ", trim(failureText()); stop 1
  end if
  ! the diagnostic tallies share their place: the others are refused while this one is on
  call initializeState(status)
  call specifyParameters(mc, status = status, computePathLengths = .true.)
  print '(a, l2, 1x, a)', "exclusive   ", stateIsFailure(status), trim(failureText())
  call initializeState(status)
  randoms = new_RandomNumberSequence(seed = (/ 7, 3 /))
  photons = new_PhotonStream(0.5, 30., numberOfPhotons = nPhotons, randomNumbers = randoms, status = status)
  call computeRadiativeTransfer(mc, randoms, photons, status)
  if(stateIsFailure(status)) then
    print *, "computeRadiativeTransfer failed: ", trim(failureText()); stop 1
  end if
  call initializeState(status)
  call reportResults(mc, status = status, pathHistogramPathDown = wrong)
  print '(a, l2, 1x, a)', "wrongsize   ", stateIsFailure(status), trim(failureText())
  call initializeState(status)
  call reportResults(mc, status = status, pathHistogramUp = up, pathHistogramPathUp = pathUp, pathHistogramDown = down, &
                     pathHistogramPathDown = pathDown)
  if(stateIsFailure(status)) then
    print *, "reportResults failed: ", trim(failureText()); stop 1
  end if
  print '(a, 25es16.8)', "binUp       ", up
  print '(a, 25es16.8)', "binPathUp   ", pathUp
  print '(a, 25es16.8)', "binDown     ", down
  print '(a, 25es16.8)', "binPathDown ", pathDown
  total = sum(dble(up))
  do k = 1, 3
    ratio(k) = 0.d0
    do b = 1, nBins + 1
      if(up(b) > 0.) ratio(k) = ratio(k) + dble(up(b)) * exp(-dble(absorption(k)) * dble(pathUp(b)) / dble(up(b)))
    end do
    ratio(k) = ratio(k) / total
  end do
  print '(a, 3es20.12)', "ratioUp     ", ratio
  ! switched off again: the arrays are gone
  call specifyParameters(mc, status = status, pathHistogramEdges = edges(1:0))
  call initializeState(status)
  call reportResults(mc, status = status, pathHistogramDown = down)
  print '(a, l2)', "offagain    ", stateIsFailure(status)
  call finalize_Integrator(mc)
  print '(a)', "pathHistogramTest done"
contains
  ! the oldest message of the status object (the probes start from a fresh one)
  function failureText() result(text)
    character(len = 256) :: text
    call firstMessage(status)
    text = getCurrentMessage(status)
  end function failureText
end program pathHistogramTest
