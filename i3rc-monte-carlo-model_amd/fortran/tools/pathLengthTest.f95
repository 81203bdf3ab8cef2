! Path-length moments through the Fortran shell: specifyParameters(computePathLengths = .true.) and reportResults(pathLengthUp =,
! pathLengthSquaredUp =, pathLengthDown =, pathLengthSquaredDown =) on a small cloud over a reflecting surface, irregular layers.
! Prints the four arrays, column after column, and the two domain mean paths -- sum(path) / sum(flux), summed in double precision --
! (tests/test_gpu_path_lengths.py runs the same photons through the Python mirror), and what the shell answers when the arrays are
! asked for without having been computed, or into an array of the wrong shape.
program pathLengthTest
  use ErrorMessages
  use RandomNumbers
  use scatteringPhaseFunctions
  use opticalProperties
  use monteCarloIllumination
  use monteCarloRadiativeTransfer
  implicit none
  integer, parameter :: nx = 4, ny = 2, nz = 6, nPhotons = 50000
  type(ErrorMessage)         :: status
  type(domain)               :: cloud
  type(integrator)           :: mc
  type(randomNumberSequence) :: randoms
  type(photonStream)         :: photons
  type(phaseFunction)        :: hg
  type(phaseFunctionTable)   :: table
  real    :: ext(nx, ny, nz), ssa(nx, ny, nz), up1(nx, ny), up2(nx, ny), down1(nx, ny), down2(nx, ny), wrong(nx, ny + 1)
  real    :: fluxUp(nx, ny), fluxDown(nx, ny)
  integer :: idx(nx, ny, nz), i, j, k

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

  ! asked for before it is switched on
  randoms = new_RandomNumberSequence(seed = (/ 7, 3 /))
  photons = new_PhotonStream(0.5, 30., numberOfPhotons = nPhotons, randomNumbers = randoms, status = status)
  call computeRadiativeTransfer(mc, randoms, photons, status)
  call finalize_PhotonStream(photons)
  call initializeState(status)
  call reportResults(mc, status = status, pathLengthUp = up1)
  print '(a, l2, 1x, a)', "unavailable ", stateIsFailure(status), trim(failureText())
  call initializeState(status)

  call specifyParameters(mc, status = status, computePathLengths = .true.)
  if(stateIsFailure(status)) then
    print *, "specifyParameters(computePathLengths) failed"; stop 1
  end if
  ! the three diagnostic tallies share their place: the others are refused while this one is on
  call initializeState(status)
  call specifyParameters(mc, status = status, computeActinicFlux = .true.)
  print '(a, l2, 1x, a)', "exclusive   ", stateIsFailure(status), trim(failureText())
  call initializeState(status)
  randoms = new_RandomNumberSequence(seed = (/ 7, 3 /))
  photons = new_PhotonStream(0.5, 30., numberOfPhotons = nPhotons, randomNumbers = randoms, status = status)
  call computeRadiativeTransfer(mc, randoms, photons, status)
  if(stateIsFailure(status)) then
    print *, "computeRadiativeTransfer failed: ", trim(failureText()); stop 1
  end if
  call initializeState(status)
  call reportResults(mc, status = status, pathLengthSquaredDown = wrong)
  print '(a, l2, 1x, a)', "wrongshape  ", stateIsFailure(status), trim(failureText())
  call initializeState(status)
  call reportResults(mc, fluxUp = fluxUp, fluxDown = fluxDown, status = status, pathLengthUp = up1, pathLengthSquaredUp = up2, &
                     pathLengthDown = down1, pathLengthSquaredDown = down2)
  if(stateIsFailure(status)) then
    print *, "reportResults failed: ", trim(failureText()); stop 1
  end if
  print '(a, 8es16.8)', "pathUp1     ", ((up1(i, j),   i = 1, nx), j = 1, ny)
  print '(a, 8es16.8)', "pathUp2     ", ((up2(i, j),   i = 1, nx), j = 1, ny)
  print '(a, 8es16.8)', "pathDown1   ", ((down1(i, j), i = 1, nx), j = 1, ny)
  print '(a, 8es16.8)', "pathDown2   ", ((down2(i, j), i = 1, nx), j = 1, ny)
  print '(a, 2es20.12)', "meanPath    ", sum(dble(up1)) / sum(dble(fluxUp)), sum(dble(down1)) / sum(dble(fluxDown))
  ! switched off again: the arrays are gone
  call specifyParameters(mc, status = status, computePathLengths = .false.)
  call initializeState(status)
  call reportResults(mc, status = status, pathLengthDown = down1)
  print '(a, l2)', "offagain    ", stateIsFailure(status)
  call finalize_Integrator(mc)
  print '(a)', "pathLengthTest done"
contains
  ! the oldest message of the status object (the probes start from a fresh one)
  function failureText() result(text)
    character(len = 256) :: text
    call firstMessage(status)
    text = getCurrentMessage(status)
  end function failureText
end program pathLengthTest
